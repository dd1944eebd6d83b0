/*
 * kmerutils.hpp -- host side above the C-ABI (include/kmu.h), in C++ because the reference is compiled code (Rust) whose
 * toolchain is absent from this image.  It mirrors the reference's own interface for the hot path -- same type and method
 * names, same argument meaning, errors where the reference panics -- so that code written against jean-pierreBoth/kmerutils
 * (and the tests in tests/cpp, which follow the reference's tests) reads the same.  Header-only, C++17, links libkmu.so only.
 *
 *   base          Sequence                                   src/base/sequence.rs:14-320
 *                 Kmer32bit / Kmer16b32bit / Kmer64bit       src/base/kmer32bit.rs, kmer16b32bit.rs, kmer64bit.rs
 *                 KmerT / CompressedKmerT / KmerBuilder      src/base/kmertraits.rs:14-52
 *                 KmerGenerator::generate_kmer               src/base/kmergenerator.rs:117-239
 *   aautils       SequenceAA, KmerAA32bit, KmerAA64bit       src/aautils/kmeraa.rs:146-484
 *   sketching     SeqSketcherParams, SketchAlgo, DataType    src/sketcharg.rs:13-78
 *                 SeqSketcherT (trait)                       src/sketching/setsketchert.rs:54-80
 *                 ProbHash3aSketch / SuperHashSketch / SuperHash2Sketch   setsketchert.rs:85-336, 904-1046
 *                 OptDensHashSketch / RevOptDensHashSketch                setsketchert.rs:343-599
 *                 HyperLogLogSketch, SetSketchParams, HllSeqsThreading    setsketchert.rs:600-896
 *                 SeqSketcher                                src/sketching/seqsketchjaccard.rs:117-415
 *                 jaccard_index_probminhash3a, probminhash_get_jaccard_objects, compute_*_jaccard
 *                                                            seqsketchjaccard.rs:58-108, 423-495
 *                 BlockSeqSketcher, BlockSketched, BlockSketchedSeq, DistBlockSketched
 *                                                            src/sketching/seqblocksketch.rs:38-227, 419-440
 *                 MinInvHashCountKmer, minhash_distance      src/sketching/minhash.rs:134-340
 *   anchors       AnchorsGeneratorParameters, SliceAnchor, ReadAnchors, gen_read_anchors   src/anchor.rs:29-329
 *                 AnchorMatch, match_read_anchors (the join behind redis_dump's index)     src/anchor.rs:187-197
 *                 AnchorIndex (that index as a resident object, with a repeat mask)        src/anchor.rs:187-197
 *                 Overlap, anchor_overlaps, read_overlaps (read pairs from matched slices)  (beyond the reference)
 *                 Components, components, components_knn, ReadClusters, read_clusters       (beyond the reference)
 *                                                            (connected components of overlap records / neighbour lists)
 *                 chain_align, align_chains, read_alignments, paf_line (banded edit distance and matches per chain; PAF text)
 *                 ChainCigars, chain_cigar, cigar_chains, cigar_string, paf_line with cg:Z: (the path of every chain's alignment)
 *                 ChainPileups, chain_pileup, pileup_chains, PileCalls, pile_call (per-base votes of the paths, calls per base and read)
 *                 InsPlan, pile_ins_plan, ChainInsertions, chain_pile_ins, ConsensusReads, pile_consensus, correct_chains, correct_reads
 *                 (the inserted letters and the corrected reads)
 *                 PileSegments, pile_segments, extract_ranges, pile_consensus_pos, trim_reads, correct_trim_chains, correct_trim_reads
 *                 (supported segments of every read, chimera splits and trimmed reads)
 *                 GraphParams, OverlapClasses, sg_classify, OverlapGraph, overlap_graph, read_graph, unitig_labels, gfa_line
 *                 (overlap classes, contained reads, the transitively reduced string graph)
 *                 Unitigs, sg_unitigs, UnitigSequences, unitig_sequences, ReadUnitigs, read_unitigs, unitig_gfa_line
 *                 (the ordered reads of every unitig, their coordinates and the unitig's bases)
 *                 CleanGraph, sg_clean, clean_graph, layout_reads (tips removed and simple bubbles popped before the layout)
 *                 UnitigChains, sg_unitig_chains, unitig_read_chains, PolishedUnitigs, polish_unitigs
 *                 (every read mapped onto its unitig from the layout, and the consensus of a unitig over its reads)
 *                 seed_chains_all, chain_rank, chain_mapq, paf_line with a rank record (every chain of every read pair; primary
 *                 and secondary chains per query read; mapping quality)
 *                 read_syncmers (closed and open syncmers of every read, in the record of read_minimizers)
 *                 seed_chains, seed_pairs, chain_hits, read_chains (one base-resolution chain per read pair from minimizer
 *                                                            hits)                          (beyond the reference)
 *   counting      KmerCountT (trait), KmerCounter, KmerCounterPool, count_kmer_threaded_one_to_many
 *                                                            src/base/kmercount.rs:48-123, 424-565, 881-974
 *                 KmerPrefilter, count_repeated_kmers (a Bloom prefilter keeps the k-mers seen once off the table)
 *   io            FASTQ reader rule, signature / count dumps src/io.rs:12-72, src/bin/datasketcher.rs:358-388,
 *                                                            seqsketchjaccard.rs:385-414, kmercount.rs:467-531
 *
 * What runs where: containers and bookkeeping on the host (as upstream); k-mer generation, canonicalisation, hashing,
 * multisets, sketches, counting, FASTQ filtering and signature comparison on the GPU through libkmu.  There is no CPU
 * implementation of those steps here: without libkmu.so / a device every call throws KmuError.
 *
 * A Rust closure `fhash: Fn(&Kmer) -> Kmer::Val` cannot cross an FFI.  Two ways to say what it is:
 *   - an FHash constant naming one of the closures the reference's own callers use (evaluated on the device), e.g.
 *     `kmer_revcomp_hash_fn` for `|kmer| intNN_hash(kmer.reverse_complement().min(*kmer).0)`;
 *   - any C++ callable `Val(const Kmer&)`: the k-mers are generated on the device, the callable is evaluated on the host,
 *     multiset + sketch run on the device (kmu_sketch_hashed, the fallback of include/kmu.h).
 */
#ifndef KMERUTILS_HPP
#define KMERUTILS_HPP

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <charconv>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <memory>
#include <mutex>
#include <optional>
#include <stdexcept>
#include <string>
#include <string_view>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "kmu.h"

namespace kmerutils {

// =====================================================================================================================
// errors + device context
// =====================================================================================================================

/// What the reference reports by panicking (bad k, empty sequence, non-ACGT byte ...) arrives here as an exception.
class KmuError : public std::runtime_error {
  public:
    KmuError(int status, const std::string &what) : std::runtime_error(what), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

/// One HIP device + stream (kmu_ctx).  Use from one thread at a time.
class Context {
  public:
    explicit Context(int device_id = 0) {
        kmu_device_cfg cfg{};
        cfg.device_id = device_id;
        int rc = kmu_create(&cfg, &ctx_);
        if (rc != KMU_OK) throw KmuError(rc, std::string("kmu_create: ") + kmu_last_error(nullptr));
    }
    ~Context() {
        if (ctx_) kmu_destroy(ctx_);
    }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;

    kmu_ctx *raw() const { return ctx_; }
    void check(int rc) const {
        if (rc != KMU_OK) throw KmuError(rc, kmu_last_error(ctx_));
    }
    /// process-wide context on device 0, created on first use (the reference has no such object: rayon's global pool
    /// plays that role there)
    static Context &global() {
        static Context ctx(0);
        return ctx;
    }

  private:
    kmu_ctx *ctx_ = nullptr;
};

/// A buffer in the memory of the context's GPU (kmu_dev_alloc): for data that should cross PCIe once.
class DeviceBuffer {
  public:
    DeviceBuffer() = default;
    DeviceBuffer(Context &ctx, uint64_t bytes) : ctx_(&ctx), bytes_(bytes) { ctx.check(kmu_dev_alloc(ctx.raw(), bytes, &p_)); }
    ~DeviceBuffer() { release(); }
    DeviceBuffer(DeviceBuffer &&o) noexcept : ctx_(o.ctx_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept {
        if (this != &o) {
            release();
            ctx_ = o.ctx_; p_ = o.p_; bytes_ = o.bytes_;
            o.p_ = nullptr;
        }
        return *this;
    }
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    void *data() const { return p_; }
    template <class T> T *as() const { return static_cast<T *>(p_); }
    uint64_t bytes() const { return bytes_; }
    void upload(const void *src, uint64_t n, uint64_t at = 0) { ctx_->check(kmu_copy_to_device(ctx_->raw(), as<uint8_t>() + at, src, n)); }
    void download(void *dst, uint64_t n, uint64_t from = 0) const { ctx_->check(kmu_copy_to_host(ctx_->raw(), dst, as<uint8_t>() + from, n)); }

  private:
    void release() {
        if (p_) (void) kmu_dev_free(ctx_->raw(), p_);
        p_ = nullptr;
    }
    Context *ctx_ = nullptr;
    void *p_ = nullptr;
    uint64_t bytes_ = 0;
};

// =====================================================================================================================
// base: Sequence
// =====================================================================================================================

/// 2-bit alphabet, src/base/alphabet.rs:119-127 (A0 C1 G2 T3, case-insensitive)
struct Alphabet2b {
    static bool is_valid_base(uint8_t c) {
        switch (c) {
        case 'A': case 'C': case 'G': case 'T': case 'a': case 'c': case 'g': case 't': return true;
        default: return false;
        }
    }
    static uint8_t encode(uint8_t c) {
        switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: throw std::invalid_argument("Alphabet2b::encode: not a base in ACGT");  // upstream panics
        }
    }
    static uint8_t decode(uint8_t code) { return "ACGT"[code & 3]; }
};

/// Sequence::new(raw, 2): 4 bases per byte, first base in bits 7..6, tail padded with A (sequence.rs:25-106).
/// Only the 2-bit representation is on the path (KmerSeqIterator refuses the others, kmergenerator.rs:221-223).
class Sequence {
  public:
    Sequence(const uint8_t *raw, size_t n, uint8_t nb_bits = 2) : nb_bases_(n) {
        if (nb_bits != 2) throw std::invalid_argument("Sequence: only 2 bits per base are supported on this path");
        seq_.assign((n + 3) / 4, 0);
        for (size_t i = 0; i < n; i++) seq_[i >> 2] |= uint8_t(Alphabet2b::encode(raw[i]) << (6 - 2 * (i & 3)));
    }
    explicit Sequence(std::string_view s, uint8_t nb_bits = 2)
        : Sequence(reinterpret_cast<const uint8_t *>(s.data()), s.size(), nb_bits) {}

    uint8_t nb_bits_by_base() const { return 2; }
    size_t size() const { return nb_bases_; }
    size_t compressed_length() const { return seq_.size(); }
    /// the 2-bit code of base `pos` (sequence.rs:120-139)
    uint8_t get_base(size_t pos) const { return (seq_[pos >> 2] >> (6 - 2 * (pos & 3))) & 3; }
    std::vector<uint8_t> decompress() const {
        std::vector<uint8_t> out(nb_bases_);
        for (size_t i = 0; i < nb_bases_; i++) out[i] = Alphabet2b::decode(get_base(i));
        return out;
    }
    Sequence get_reverse_complement() const {
        std::vector<uint8_t> rc(nb_bases_);
        for (size_t i = 0; i < nb_bases_; i++) rc[i] = Alphabet2b::decode(3 - get_base(nb_bases_ - 1 - i));
        return Sequence(rc.data(), rc.size(), 2);
    }
    const std::vector<uint8_t> &packed() const { return seq_; }

  private:
    std::vector<uint8_t> seq_;
    size_t nb_bases_;
};

// =====================================================================================================================
// base: k-mer value types (host-side value semantics; the device computes the same values, kmu_kmer_hashes)
// =====================================================================================================================

namespace detail {
inline uint32_t bitrev32(uint32_t x) {
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    return __builtin_bswap32(x);
}
inline uint64_t bitrev64(uint64_t x) { return (uint64_t(bitrev32(uint32_t(x))) << 32) | bitrev32(uint32_t(x >> 32)); }
/// complement every base and reverse their order inside the word: !v, reverse the bits, swap the bits of each pair
inline uint32_t revcomp_word(uint32_t v) {
    uint32_t r = bitrev32(~v);
    return ((r & 0x55555555u) << 1) | ((r & 0xAAAAAAAAu) >> 1);
}
inline uint64_t revcomp_word(uint64_t v) {
    uint64_t r = bitrev64(~v);
    return ((r & 0x5555555555555555ull) << 1) | ((r & 0xAAAAAAAAAAAAAAAAull) >> 1);
}
}  // namespace detail

/// up to 14 bases in a u32, k in bits 31..28 (kmer32bit.rs:22-217).  `v` is the reference's `.0`.
struct Kmer32bit {
    using Val = uint32_t;
    static constexpr int kmu_type = KMU_KMER32BIT;
    static constexpr bool is_aa = false;
    uint32_t v = 0;

    Kmer32bit() = default;
    explicit Kmer32bit(uint32_t raw) : v(raw) {}
    static Kmer32bit build(Val val, uint8_t k) { return Kmer32bit((uint32_t(k) << 28) | val); }   // KmerBuilder
    static Kmer32bit from_raw(uint64_t raw, uint8_t) { return Kmer32bit(uint32_t(raw)); }
    static constexpr size_t get_nb_base_max() { return 14; }
    static constexpr size_t get_bitsize() { return 32; }
    uint8_t get_nb_base() const { return uint8_t(v >> 28); }
    Val get_compressed_value() const { return v & 0x0FFFFFFFu; }
    Val raw() const { return v; }
    Kmer32bit push(uint8_t base) const {
        const uint32_t k = v >> 28;
        return Kmer32bit((v & 0xF0000000u) | (((v << 2) & ((1u << (2 * k)) - 1u)) | (base & 3u)));
    }
    Kmer32bit reverse_complement() const {
        const uint32_t k = v >> 28;
        return Kmer32bit((v & 0xF0000000u) | ((detail::revcomp_word(v) >> (32 - 2 * k)) & 0x0FFFFFFFu));
    }
    std::vector<uint8_t> get_uncompressed_kmer() const {
        const int k = get_nb_base();
        std::vector<uint8_t> s(k);
        for (int i = 0; i < k; i++) s[i] = Alphabet2b::decode(uint8_t(v >> (2 * (k - 1 - i))));
        return s;
    }
    /// Ord: number of bases first, then value (kmer32bit.rs:47-55)
    bool operator<(const Kmer32bit &o) const {
        return (v >> 28) != (o.v >> 28) ? (v >> 28) < (o.v >> 28) : get_compressed_value() < o.get_compressed_value();
    }
    bool operator==(const Kmer32bit &o) const { return v == o.v; }
    Kmer32bit min(const Kmer32bit &o) const { return o < *this ? o : *this; }
};

/// exactly 16 bases in a u32 (kmer16b32bit.rs:21-132)
struct Kmer16b32bit {
    using Val = uint32_t;
    static constexpr int kmu_type = KMU_KMER16B32BIT;
    static constexpr bool is_aa = false;
    uint32_t v = 0;

    Kmer16b32bit() = default;
    explicit Kmer16b32bit(uint32_t raw) : v(raw) {}
    static Kmer16b32bit build(Val val, uint8_t) { return Kmer16b32bit(val); }
    static Kmer16b32bit from_raw(uint64_t raw, uint8_t) { return Kmer16b32bit(uint32_t(raw)); }
    static constexpr size_t get_nb_base_max() { return 16; }
    static constexpr size_t get_bitsize() { return 32; }
    uint8_t get_nb_base() const { return 16; }
    Val get_compressed_value() const { return v; }
    Val raw() const { return v; }
    Kmer16b32bit push(uint8_t base) const { return Kmer16b32bit((v << 2) | (base & 3u)); }
    Kmer16b32bit reverse_complement() const { return Kmer16b32bit(detail::revcomp_word(v)); }
    std::vector<uint8_t> get_uncompressed_kmer() const {
        std::vector<uint8_t> s(16);
        for (int i = 0; i < 16; i++) s[i] = Alphabet2b::decode(uint8_t(v >> (2 * (15 - i))));
        return s;
    }
    bool operator<(const Kmer16b32bit &o) const { return v < o.v; }
    bool operator==(const Kmer16b32bit &o) const { return v == o.v; }
    Kmer16b32bit min(const Kmer16b32bit &o) const { return o < *this ? o : *this; }
};

/// up to 31 bases: (u64 value, u8 k) (kmer64bit.rs:24-172; k = 32 is broken upstream)
struct Kmer64bit {
    using Val = uint64_t;
    static constexpr int kmu_type = KMU_KMER64BIT;
    static constexpr bool is_aa = false;
    uint64_t v = 0;   // `.0`
    uint8_t k = 0;    // `.1`

    Kmer64bit() = default;
    Kmer64bit(uint64_t val, uint8_t nb) : v(val), k(nb) {}
    static Kmer64bit build(Val val, uint8_t nb) { return Kmer64bit(val, nb); }
    static Kmer64bit from_raw(uint64_t raw, uint8_t nb) { return Kmer64bit(raw, nb); }
    static constexpr size_t get_nb_base_max() { return 32; }
    static constexpr size_t get_bitsize() { return 64; }
    uint8_t get_nb_base() const { return k; }
    Val get_compressed_value() const { return v; }
    Val raw() const { return v; }
    Kmer64bit push(uint8_t base) const { return Kmer64bit(((v << 2) & ((1ull << (2 * k)) - 1ull)) | (base & 3ull), k); }
    Kmer64bit reverse_complement() const { return Kmer64bit(detail::revcomp_word(v) >> (64 - 2 * k), k); }
    std::vector<uint8_t> get_uncompressed_kmer() const {
        std::vector<uint8_t> s(k);
        for (int i = 0; i < k; i++) s[i] = Alphabet2b::decode(uint8_t(v >> (2 * (k - 1 - i))));
        return s;
    }
    bool operator<(const Kmer64bit &o) const { return k != o.k ? k < o.k : v < o.v; }
    bool operator==(const Kmer64bit &o) const { return v == o.v && k == o.k; }
    Kmer64bit min(const Kmer64bit &o) const { return o < *this ? o : *this; }
};

// ---- amino acids (src/aautils/kmeraa.rs) -----------------------------------------------------------------------------

/// aautils::kmeraa::Alphabet: 5 bits, upper case only (kmeraa.rs:29-139)
struct AlphabetAA {
    static constexpr uint8_t get_nb_bits() { return 5; }
    static bool is_valid_base(uint8_t c) { return code_of(c) != 0; }
    static uint8_t encode(uint8_t c) {
        const uint8_t code = code_of(c);
        if (!code) throw std::invalid_argument("aautils Alphabet::encode: not an amino acid letter");
        return code;
    }

  private:
    static uint8_t code_of(uint8_t c) {
        // A1 C2 D3 E4 F5 G6 H7 I8 K9 L10 M11 N12 P13 Q15 R16 S17 T18 V19 W20 Y21 (kmeraa.rs:86-107)
        static const char *letters = "ACDEFGHIKLMNPQRSTVWY";
        static const uint8_t codes[20] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21};
        for (int i = 0; i < 20; i++)
            if (uint8_t(letters[i]) == c) return codes[i];
        return 0;
    }
};

/// SequenceAA: one byte per residue, un-encoded (kmeraa.rs:404-484)
class SequenceAA {
  public:
    explicit SequenceAA(std::string_view s) : seq_(s.begin(), s.end()) {}
    SequenceAA(const uint8_t *raw, size_t n) : seq_(raw, raw + n) {}
    static SequenceAA from_str(std::string_view s) { return SequenceAA(s); }
    /// drops the bytes that are not amino-acid letters (kmeraa.rs:447-456)
    static SequenceAA new_filtered(const uint8_t *raw, size_t n) {
        SequenceAA s(std::string_view{});
        for (size_t i = 0; i < n; i++)
            if (AlphabetAA::is_valid_base(raw[i])) s.seq_.push_back(raw[i]);
        return s;
    }
    size_t len() const { return seq_.size(); }
    size_t size() const { return seq_.size(); }
    const std::vector<uint8_t> &bytes() const { return seq_; }

  private:
    std::vector<uint8_t> seq_;
};

template <class V, int TYPE, int KMAX> struct KmerAAbits {
    using Val = V;
    static constexpr int kmu_type = TYPE;
    static constexpr bool is_aa = true;
    V v = 0;
    uint8_t k = 0;

    KmerAAbits() = default;
    KmerAAbits(V val, uint8_t nb) : v(val), k(nb) {}
    static KmerAAbits build(V val, uint8_t nb) { return KmerAAbits(val, nb); }
    static KmerAAbits from_raw(uint64_t raw, uint8_t nb) { return KmerAAbits(V(raw), nb); }
    static constexpr size_t get_nb_base_max() { return KMAX; }
    static constexpr size_t get_bitsize() { return 8 * sizeof(V); }
    uint8_t get_nb_base() const { return k; }
    V get_compressed_value() const { return v; }
    V raw() const { return v; }
    /// `c` is the residue letter: push encodes (kmeraa.rs:303-306)
    KmerAAbits push(uint8_t c) const {
        return KmerAAbits(V(((v << 5) & ((V(1) << (5 * k)) - 1)) | AlphabetAA::encode(c)), k);
    }
    KmerAAbits reverse_complement() const { throw std::logic_error("KmerAA: reverse_complement makes no sense"); }  // :315
    bool operator<(const KmerAAbits &o) const { return k != o.k ? k < o.k : v < o.v; }
    bool operator==(const KmerAAbits &o) const { return v == o.v && k == o.k; }
};
using KmerAA32bit = KmerAAbits<uint32_t, KMU_KMERAA32BIT, 6>;    // kmeraa.rs:146-274
using KmerAA64bit = KmerAAbits<uint64_t, KMU_KMERAA64BIT, 12>;   // kmeraa.rs:280-397

// =====================================================================================================================
// fhash: the closures of the reference's callers, by name
// =====================================================================================================================

enum class FHash : int {
    identity_raw = KMU_FHASH_IDENTITY_RAW,       // |kmer| kmer.0
    value_masked = KMU_FHASH_VALUE_MASKED,       // |kmer| kmer.get_compressed_value() & mask
    canon_raw = KMU_FHASH_CANON_RAW,             // |kmer| kmer.reverse_complement().min(*kmer).0
    canon_invhash = KMU_FHASH_CANON_INVHASH,     // |kmer| intNN_hash(kmer.reverse_complement().min(*kmer).0)
    invhash_raw = KMU_FHASH_INVHASH_RAW,         // |kmer| intNN_hash(kmer.0)
    canon_value = KMU_FHASH_CANON_VALUE,         // |kmer| min(kmer, revcomp).get_compressed_value()
    canon_nthash = KMU_FHASH_CANON_NTHASH,
    canon_nthash_8b = KMU_FHASH_CANON_NTHASH_8B,
};
/// the names the reference's tests give these closures (seqsketchjaccard.rs:768-775, aautils/setsketchert.rs:1235-1241)
inline constexpr FHash kmer_revcomp_hash_fn = FHash::canon_invhash;
inline constexpr FHash kmer_identity = FHash::identity_raw;
inline constexpr FHash kmer_hash_fn = FHash::value_masked;

// =====================================================================================================================
// gathering sequences into the (bytes, offsets) form of the C-ABI
// =====================================================================================================================

namespace detail {

struct Batch {
    std::vector<uint8_t> bytes;
    std::vector<uint64_t> offsets;         // in bases / residues, n + 1 (always on the host: sizes, block layouts)
    std::vector<uint64_t> packed_offsets;  // byte offset of every packed sequence (DNA)
    int input_kind = KMU_INPUT_ASCII;
    // device-resident batch (reads left on the GPU by the FASTX reader): these pointers are used instead of `bytes` and
    // the host `offsets`; the offsets index the whole device array, so a range of reads needs no copy
    const uint8_t *dev_bytes = nullptr;
    const uint64_t *dev_offsets = nullptr;
    bool on_device() const { return dev_bytes != nullptr; }
    int mem() const { return on_device() ? KMU_MEM_DEVICE : KMU_MEM_HOST; }
    const uint8_t *bytes_ptr() const { return on_device() ? dev_bytes : bytes.data(); }
    const uint64_t *offsets_ptr() const { return on_device() ? dev_offsets : offsets.data(); }
    uint32_t n() const { return uint32_t(offsets.size() - 1); }
    const uint64_t *packed_ptr() const { return input_kind == KMU_INPUT_PACKED2 ? packed_offsets.data() : nullptr; }
};

inline Batch gather(const std::vector<const Sequence *> &vseq) {
    Batch b;
    b.input_kind = KMU_INPUT_PACKED2;
    b.offsets.assign(1, 0);
    for (const Sequence *s : vseq) {
        b.packed_offsets.push_back(b.bytes.size());
        b.bytes.insert(b.bytes.end(), s->packed().begin(), s->packed().end());
        b.offsets.push_back(b.offsets.back() + s->size());
    }
    if (b.packed_offsets.empty()) b.packed_offsets.push_back(0);
    b.bytes.resize(b.bytes.size() + 16, 0);
    return b;
}

inline Batch gather(const std::vector<const SequenceAA *> &vseq) {
    Batch b;
    b.offsets.assign(1, 0);
    for (const SequenceAA *s : vseq) {
        b.bytes.insert(b.bytes.end(), s->bytes().begin(), s->bytes().end());
        b.offsets.push_back(b.offsets.back() + s->len());
    }
    b.bytes.resize(b.bytes.size() + 16, 0);
    return b;
}

/// a packed (Sequence) batch as ASCII, for the entry points that take unpacked bases only
inline Batch unpacked(const Batch &b) {
    if (b.input_kind != KMU_INPUT_PACKED2) return b;
    Batch a;
    a.offsets = b.offsets;
    a.bytes.resize(b.offsets.back() + 16, 0);
    for (uint32_t i = 0; i < b.n(); i++)
        for (uint64_t p = 0, len = b.offsets[i + 1] - b.offsets[i]; p < len; p++)
            a.bytes[b.offsets[i] + p] = Alphabet2b::decode(uint8_t(b.bytes[b.packed_offsets[i] + (p >> 2)] >> (6 - 2 * (p & 3))));
    return a;
}

template <class Seq> std::vector<const Seq *> pointers(const std::vector<Seq> &v) {
    std::vector<const Seq *> p;
    p.reserve(v.size());
    for (const Seq &s : v) p.push_back(&s);
    return p;
}

// ---- the marshalling steps of the wrappers below, each written once; where kmerutils_amd/lib.py has the same step, under its name
// there -------------------------------------------------------------------------------------------------

/// An empty vector has no address worth passing.  ptr(v): the base of v, or a spare element of its type where v is empty, for
/// the arrays the C-ABI requires (lib.py's _ptrs); opt(v): the base of v, or null where v is empty, for the optional ones.
/// An output of zero elements is sized exactly and passed through ptr like any other array.
template <class T> inline T spare_element{};
template <class T> const T *ptr(const std::vector<T> &v) { return v.empty() ? &spare_element<T> : v.data(); }
template <class T> T *ptr(std::vector<T> &v) { return v.empty() ? &spare_element<T> : v.data(); }
template <class T> const T *opt(const std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }
template <class T> T *opt(std::vector<T> &v) { return v.empty() ? nullptr : v.data(); }

/// Count, allocate, call again (lib.py's _two_calls).  `call(write, cap, &total)` runs once with write == false and cap 0 -- it
/// passes null outputs then -- `alloc(total)` sizes the outputs exactly, and the second call gets that capacity.  `always`:
/// whether the second call is made for a total of 0 (it is where it also writes offsets or summaries).  Returns the total.
template <class Alloc, class Call> uint64_t two_calls(Context &ctx, bool always, Alloc alloc, Call call) {
    uint64_t total = 0;
    ctx.check(call(false, uint64_t(0), &total));
    alloc(total);
    if (total || always) ctx.check(call(true, total, &total));
    return total;
}

/// the batch of a wrapper that returns host arrays: unpacked, and refused where its sequences lie on the device
inline Batch host_batch(const char *who, const Batch &batch) {
    Batch b = unpacked(batch);
    if (b.on_device()) throw std::invalid_argument(std::string(who) + " returns host arrays: it needs the sequences in host memory");
    return b;
}

/// the two batches of a chain call, as host_batch gives them; without a db batch (the self-join) db() is q (lib.py's _db_batch)
struct Sides {
    Batch q, own_db;
    bool two;
    const Batch &db() const { return two ? own_db : q; }
};
inline Sides host_sides(const char *who, const Batch &q, const Batch *db) {
    Sides s{unpacked(q), db ? unpacked(*db) : Batch(), db != nullptr};
    if (s.q.on_device() || s.db().on_device())
        throw std::invalid_argument(std::string(who) + " returns host arrays: it needs the sequences in host memory");
    return s;
}

/// the number of reads behind the offsets of a batch, which have one entry more
inline uint32_t n_reads_of(const char *who, const std::vector<uint64_t> &offsets) {
    if (offsets.empty()) throw std::invalid_argument(std::string(who) + ": the offsets of a batch have at least one entry");
    return uint32_t(offsets.size() - 1);
}

template <class Kmer> kmu_hash_params hash_params(size_t k, int fhash, int input_kind) {
    kmu_hash_params hp{};
    hp.kmer_type = Kmer::kmu_type;
    hp.kmer_size = int32_t(k);
    hp.fhash = fhash;
    hp.input_kind = input_kind;
    hp.mem = KMU_MEM_HOST;
    return hp;
}

/// the values a counter or a prefilter takes for a list of k-mers
template <class Kmer> std::vector<uint64_t> compressed_values(const std::vector<Kmer> &kmers) {
    std::vector<uint64_t> keys;
    for (const Kmer &k : kmers) keys.push_back(uint64_t(k.get_compressed_value()));
    return keys;
}

template <class Sig> constexpr int sig_type_of() {
    if constexpr (std::is_same_v<Sig, uint32_t>) return KMU_SIG_U32;
    else if constexpr (std::is_same_v<Sig, uint64_t>) return KMU_SIG_U64;
    else if constexpr (std::is_same_v<Sig, float>) return KMU_SIG_F32;
    else {
        static_assert(std::is_same_v<Sig, double>, "signature element must be u32, u64, f32 or f64");
        return KMU_SIG_F64;
    }
}

template <class Sig> std::vector<std::vector<Sig>> split_rows(const std::vector<Sig> &flat, size_t rows, size_t m) {
    std::vector<std::vector<Sig>> out(rows);
    for (size_t r = 0; r < rows; r++) out[r].assign(flat.begin() + r * m, flat.begin() + (r + 1) * m);
    return out;
}

inline kmu_sketch_params sketch_params(int algo, int kmer_type, size_t k, size_t m, int sig_type, int hasher, int fhash,
                                       int block_size, int mode, int input_kind) {
    kmu_sketch_params p{};
    p.algo = algo;
    p.kmer_type = kmer_type;
    p.kmer_size = int32_t(k);
    p.sketch_size = int32_t(m);
    p.sig_type = sig_type;
    p.hasher = hasher;
    p.fhash = fhash;
    p.block_size = block_size;
    p.mode = mode;
    p.input_kind = input_kind;
    p.mem = KMU_MEM_HOST;
    return p;
}

/// raw `.0` of every k-mer of every sequence, generated on the device (KmerSeqIterator::next, kmergenerator.rs:75-106)
template <class Kmer> std::vector<std::vector<Kmer>> device_kmers(Context &ctx, const Batch &b, size_t k) {
    if (b.on_device()) throw std::invalid_argument("k-mer lists / host closures need the sequences in host memory");
    const kmu_hash_params hp = hash_params<Kmer>(k, KMU_FHASH_IDENTITY_RAW, b.input_kind);
    std::vector<uint64_t> raw(b.offsets.back(), 0);
    ctx.check(kmu_kmer_hashes(ctx.raw(), &hp, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), ptr(raw)));
    std::vector<std::vector<Kmer>> out(b.n());
    for (uint32_t i = 0; i < b.n(); i++) {
        const uint64_t len = b.offsets[i + 1] - b.offsets[i];
        if (len < k) continue;   // a sequence shorter than k yields nothing (kmergenerator.rs:98-99)
        out[i].reserve(len - k + 1);
        for (uint64_t p = 0; p + k <= len; p++) out[i].push_back(Kmer::from_raw(raw[b.offsets[i] + p], uint8_t(k)));
    }
    return out;
}

/// rows of signatures for a batch, row-major in `flat` (resized to rows * m; a caller that sketches pack after pack keeps
/// one such buffer), either with a device-side closure (FHash) or a host callable.  Returns the number of rows.
template <class Kmer, class Sig, class F>
size_t run_sketch_flat(Context &ctx, const Batch &b, int algo, size_t k, size_t m, int hasher, F fhash, int mode,
                       std::vector<Sig> &flat, uint32_t flags = 0) {
    const size_t rows = mode == KMU_MODE_ALL_SEQS ? 1 : b.n();
    flat.resize(std::max<size_t>(rows, 1) * m);
    if constexpr (std::is_same_v<F, FHash>) {
        kmu_sketch_params p =
            sketch_params(algo, Kmer::kmu_type, k, m, sig_type_of<Sig>(), hasher, int(fhash), 0, mode, b.input_kind);
        p.flags = flags;
        p.mem = b.mem();
        if (b.on_device()) {   // reads already on the GPU: only the signatures cross PCIe
            DeviceBuffer d_sig(ctx, flat.size() * sizeof(Sig));
            ctx.check(kmu_sketch(ctx.raw(), &p, b.dev_bytes, b.dev_offsets, nullptr, b.n(), nullptr, d_sig.data(), nullptr));
            d_sig.download(flat.data(), flat.size() * sizeof(Sig));
        } else {
            ctx.check(kmu_sketch(ctx.raw(), &p, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), nullptr, flat.data(),
                                 nullptr));
        }
    } else {
        static_assert(std::is_invocable_r_v<typename Kmer::Val, F, const Kmer &>, "fhash must be Val(const Kmer&)");
        using Val = typename Kmer::Val;
        auto kmers = device_kmers<Kmer>(ctx, b, k);
        std::vector<Val> hashed;
        std::vector<uint64_t> off(1, 0);
        for (const auto &seq : kmers) {
            for (const Kmer &km : seq) hashed.push_back(fhash(km));
            off.push_back(hashed.size());
        }
        kmu_sketch_params p = sketch_params(algo, Kmer::kmu_type, k, m, sig_type_of<Sig>(), hasher, KMU_FHASH_IDENTITY_RAW, 0,
                                            mode, KMU_INPUT_ASCII);
        p.flags = flags;
        ctx.check(kmu_sketch_hashed(ctx.raw(), &p, ptr(hashed), off.data(), b.n(), flat.data(), nullptr));
    }
    return rows;
}

/// one ALL_SEQS signature per inner list of `groups`, in one library call (kmu_sketch_groups)
template <class Kmer, class Sig, class Seq>
std::vector<std::vector<Sig>> run_sketch_groups(Context &ctx, const std::vector<std::vector<const Seq *>> &groups, int algo, size_t k,
                                                size_t m, int sig_type, int hasher, FHash fhash, uint32_t flags = 0) {
    std::vector<const Seq *> all;
    std::vector<uint64_t> group_offsets(1, 0);
    for (const auto &g : groups) {
        all.insert(all.end(), g.begin(), g.end());
        group_offsets.push_back(all.size());
    }
    const Batch b = gather(all);
    kmu_sketch_params p = sketch_params(algo, Kmer::kmu_type, k, m, sig_type, hasher, int(fhash), 0, KMU_MODE_ALL_SEQS, b.input_kind);
    p.flags = flags;
    std::vector<Sig> flat(groups.size() * m);
    ctx.check(kmu_sketch_groups(ctx.raw(), &p, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), group_offsets.data(),
                                uint32_t(groups.size()), ptr(flat)));
    return split_rows(flat, groups.size(), m);
}

template <class Kmer, class Sig, class F>
std::vector<std::vector<Sig>> run_sketch(Context &ctx, const Batch &b, int algo, size_t k, size_t m, int hasher, F fhash,
                                         int mode, uint32_t flags = 0) {
    std::vector<Sig> flat;
    const size_t rows = run_sketch_flat<Kmer, Sig>(ctx, b, algo, k, m, hasher, fhash, mode, flat, flags);
    return split_rows(flat, rows, m);
}

}  // namespace detail

// =====================================================================================================================
// base: KmerGenerator
// =====================================================================================================================

/// KmerGenerator::new(k).generate_kmer(&seq) -> Vec<Kmer>: all L - k + 1 forward k-mers (kmergenerator.rs:117-239)
template <class Kmer> class KmerGenerator {
  public:
    explicit KmerGenerator(uint8_t kmer_size, Context &ctx = Context::global()) : k_(kmer_size), ctx_(ctx) {}
    std::vector<Kmer> generate_kmer(const Sequence &seq) const {
        return std::move(detail::device_kmers<Kmer>(ctx_, detail::gather(std::vector<const Sequence *>{&seq}), k_)[0]);
    }
    std::vector<Kmer> generate_kmer(const SequenceAA &seq) const {
        return std::move(detail::device_kmers<Kmer>(ctx_, detail::gather(std::vector<const SequenceAA *>{&seq}), k_)[0]);
    }
    /// generate_kmer_in_range(&seq, begin, end) (kmergenerator.rs:169-174; kmeraa.rs:667-672): the k-mers inside bases
    /// [begin, end).  A bad range throws KmuError(KMU_E_BAD_ARG) where the reference unwraps set_range's Err.
    template <class Seq> std::vector<Kmer> generate_kmer_in_range(const Seq &seq, size_t begin, size_t end) const {
        if (begin >= end) throw KmuError(KMU_E_BAD_ARG, "KmerGenerationPattern bad range for kmer iteration");  // kmergenerator.rs:284-286
        const detail::Batch b = detail::gather(std::vector<const Seq *>{&seq});
        const kmu_hash_params hp = detail::hash_params<Kmer>(k_, KMU_FHASH_IDENTITY_RAW, b.input_kind);
        std::vector<uint64_t> raw(std::max<uint64_t>(b.offsets.back(), 1), 0);
        const uint64_t rb = begin, re = end;
        ctx_.check(kmu_kmer_hashes_range(ctx_.raw(), &hp, b.bytes.data(), b.offsets.data(), b.packed_ptr(), 1, &rb, &re, raw.data()));
        std::vector<Kmer> out;
        for (uint64_t p = begin; p + k_ <= end; p++) out.push_back(Kmer::from_raw(raw[p], k_));
        return out;
    }
    /// generate_weighted_kmer(&seq) -> FnvHashMap<Kmer, u32> (kmergenerator.rs:176-181): distinct k-mers with multiplicities,
    /// counted on the device (kmu_kmer_distribution); returned as (k-mer, count) pairs in no particular order
    template <class Seq> std::vector<std::pair<Kmer, uint32_t>> generate_weighted_kmer(const Seq &seq) const {
        const detail::Batch b = detail::gather(std::vector<const Seq *>{&seq});
        const kmu_hash_params hp = detail::hash_params<Kmer>(k_, KMU_FHASH_IDENTITY_RAW, b.input_kind);
        uint64_t n = 0;
        ctx_.check(kmu_kmer_distribution(ctx_.raw(), &hp, b.bytes.data(), b.offsets.data(), b.packed_ptr(), 1, nullptr, nullptr, 0,
                                         nullptr, &n));
        std::vector<uint64_t> kk(std::max<uint64_t>(n, 1));
        std::vector<uint32_t> cc(std::max<uint64_t>(n, 1));
        ctx_.check(kmu_kmer_distribution(ctx_.raw(), &hp, b.bytes.data(), b.offsets.data(), b.packed_ptr(), 1, kk.data(), cc.data(), n,
                                         nullptr, &n));
        std::vector<std::pair<Kmer, uint32_t>> out;
        out.reserve(n);
        for (uint64_t i = 0; i < n; i++) out.emplace_back(Kmer::from_raw(kk[i], k_), cc[i]);
        return out;
    }

  private:
    uint8_t k_;
    Context &ctx_;
};

// =====================================================================================================================
// sketching: parameters and the trait
// =====================================================================================================================

enum class DataType { DNA, AA };                                              // sketcharg.rs:13-16
enum class SketchAlgo { PROB3A, SUPER, SUPER2, OPTDENS, REVOPTDENS, HLL };    // sketcharg.rs:26-33

namespace detail {
inline const char *const ALGO_NAMES[6] = {"PROB3A", "SUPER", "SUPER2", "OPTDENS", "REVOPTDENS", "HLL"};
inline const char *const DATA_NAMES[2] = {"DNA", "AA"};
/// value of "key" in a flat JSON object written by serde_json (no nesting, no escapes in what these structs hold)
inline std::string json_field(const std::string &text, const std::string &key) {
    const std::string tag = "\"" + key + "\":";
    const size_t at = text.find(tag);
    if (at == std::string::npos) throw std::runtime_error("missing field " + key);
    size_t b = at + tag.size(), e = b;
    while (e < text.size() && text[e] != ',' && text[e] != '}') e++;
    std::string v = text.substr(b, e - b);
    if (v.size() >= 2 && v.front() == '"') v = v.substr(1, v.size() - 2);
    return v;
}
inline std::string read_text_file(const std::string &path) {
    std::ifstream in(path);
    if (!in) throw std::runtime_error("reload_json could not open file " + path);
    return std::string((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}
}  // namespace detail

class SeqSketcherParams {   // sketcharg.rs:40-138
  public:
    SeqSketcherParams(size_t kmer_size, size_t sketch_size, SketchAlgo algo, DataType data_t)
        : kmer_size_(kmer_size), sketch_size_(sketch_size), algo_(algo), data_t_(data_t) {}
    size_t get_kmer_size() const { return kmer_size_; }
    size_t get_sketch_size() const { return sketch_size_; }
    SketchAlgo get_algo() const { return algo_; }
    DataType get_data_t() const { return data_t_; }
    /// dump_json: serde_json::to_writer(&self) -- {"kmer_size":8,"sketch_size":200,"algo":"PROB3A","data_t":"DNA"}
    void dump_json(const std::string &filename) const {
        std::ofstream out(filename);
        if (!out) throw std::runtime_error("SeqSketcher dump failed");
        out << "{\"kmer_size\":" << kmer_size_ << ",\"sketch_size\":" << sketch_size_ << ",\"algo\":\""
            << detail::ALGO_NAMES[int(algo_)] << "\",\"data_t\":\"" << detail::DATA_NAMES[int(data_t_)] << "\"}";
    }
    /// reload_json(dirpath): <dirpath>/sketchparams_dump.json
    static SeqSketcherParams reload_json(const std::string &dirpath) {
        const std::string text = detail::read_text_file(dirpath + "/sketchparams_dump.json");
        const std::string algo = detail::json_field(text, "algo"), data_t = detail::json_field(text, "data_t");
        int ai = -1, di = -1;
        for (int i = 0; i < 6; i++) if (algo == detail::ALGO_NAMES[i]) ai = i;
        for (int i = 0; i < 2; i++) if (data_t == detail::DATA_NAMES[i]) di = i;
        if (ai < 0 || di < 0) throw std::runtime_error("reload_json: unknown algo / data_t");
        return SeqSketcherParams(std::stoul(detail::json_field(text, "kmer_size")), std::stoul(detail::json_field(text, "sketch_size")),
                                 SketchAlgo(ai), DataType(di));
    }

  private:
    size_t kmer_size_, sketch_size_;
    SketchAlgo algo_;
    DataType data_t_;
};

/// trait SeqSketcherT<Kmer> (setsketchert.rs:54-80) and SeqSketcherAAT (aautils/setsketchert.rs:42-72) in one: the
/// sequence type follows the k-mer type.  `Sig` is the trait's associated type.
template <class Kmer, class SigT> class SeqSketcherT {
  public:
    using Sig = SigT;
    using Seq = std::conditional_t<Kmer::is_aa, SequenceAA, Sequence>;
    virtual ~SeqSketcherT() = default;
    virtual size_t get_kmer_size() const = 0;
    virtual size_t get_sketch_size() const = 0;
    virtual SketchAlgo get_algo() const = 0;
    /// one signature per sequence, row i <-> vseq[i]
    virtual std::vector<std::vector<Sig>> sketch_compressedkmer(const std::vector<const Seq *> &vseq, FHash fhash) const = 0;
    /// ONE signature for the whole list (outer length 1)
    virtual std::vector<std::vector<Sig>> sketch_compressedkmer_seqs(const std::vector<const Seq *> &vseq,
                                                                     FHash fhash) const = 0;
    /// sketch_compressedkmer_seqs of every inner list (a genome's contigs, a proteome's proteins): row g <-> groups[g], one
    /// library call for all of them (what gsearch runs file by file)
    virtual std::vector<std::vector<Sig>> sketch_compressedkmer_seqs_groups(const std::vector<std::vector<const Seq *>> &groups,
                                                                            FHash fhash) const = 0;
    // the AA trait's names for the same two calls
    std::vector<std::vector<Sig>> sketch_compressedkmeraa(const std::vector<const Seq *> &vseq, FHash fhash) const {
        return sketch_compressedkmer(vseq, fhash);
    }
    std::vector<std::vector<Sig>> sketch_compressedkmeraa_seqs(const std::vector<const Seq *> &vseq, FHash fhash) const {
        return sketch_compressedkmer_seqs(vseq, fhash);
    }
};

namespace detail {
/// shared body of the three implementers
template <class Kmer, class Sig, int ALGO> class SketcherImpl : public SeqSketcherT<Kmer, Sig> {
  public:
    using Seq = typename SeqSketcherT<Kmer, Sig>::Seq;
    SketcherImpl(const SeqSketcherParams &params, SketchAlgo algo, int hasher, Context &ctx)
        : params_(params), algo_(algo), hasher_(hasher), ctx_(ctx) {}
    size_t get_kmer_size() const override { return params_.get_kmer_size(); }
    size_t get_sketch_size() const override { return params_.get_sketch_size(); }
    SketchAlgo get_algo() const override { return algo_; }
    std::vector<std::vector<Sig>> sketch_compressedkmer(const std::vector<const Seq *> &vseq, FHash fhash) const override {
        return run(vseq, fhash, KMU_MODE_PER_SEQ);
    }
    std::vector<std::vector<Sig>> sketch_compressedkmer_seqs(const std::vector<const Seq *> &vseq,
                                                             FHash fhash) const override {
        return run(vseq, fhash, KMU_MODE_ALL_SEQS);
    }
    std::vector<std::vector<Sig>> sketch_compressedkmer_seqs_groups(const std::vector<std::vector<const Seq *>> &groups,
                                                                    FHash fhash) const override {
        return run_sketch_groups<Kmer, Sig>(ctx_, groups, ALGO, params_.get_kmer_size(), params_.get_sketch_size(),
                                            sig_type_of<Sig>(), hasher_, fhash);
    }
    /// arbitrary closure: evaluated on the host, multiset + sketch on the device
    template <class F, class = std::enable_if_t<!std::is_same_v<std::decay_t<F>, FHash>>>
    std::vector<std::vector<Sig>> sketch_compressedkmer(const std::vector<const Seq *> &vseq, F fhash) const {
        return run(vseq, fhash, KMU_MODE_PER_SEQ);
    }
    template <class F, class = std::enable_if_t<!std::is_same_v<std::decay_t<F>, FHash>>>
    std::vector<std::vector<Sig>> sketch_compressedkmer_seqs(const std::vector<const Seq *> &vseq, F fhash) const {
        return run(vseq, fhash, KMU_MODE_ALL_SEQS);
    }

  private:
    template <class F> std::vector<std::vector<Sig>> run(const std::vector<const Seq *> &vseq, F fhash, int mode) const {
        return run_sketch<Kmer, Sig>(ctx_, gather(vseq), ALGO, params_.get_kmer_size(), params_.get_sketch_size(), hasher_,
                                     fhash, mode);
    }
    SeqSketcherParams params_;
    SketchAlgo algo_;
    int hasher_;
    Context &ctx_;
};
}  // namespace detail

/// ProbHash3aSketch<Kmer>: type Sig = Kmer::Val (setsketchert.rs:85-203)
template <class Kmer> class ProbHash3aSketch : public detail::SketcherImpl<Kmer, typename Kmer::Val, KMU_ALGO_PROB3A> {
  public:
    explicit ProbHash3aSketch(const SeqSketcherParams &params, Context &ctx = Context::global())
        : detail::SketcherImpl<Kmer, typename Kmer::Val, KMU_ALGO_PROB3A>(params, SketchAlgo::PROB3A, KMU_HASHER_NOHASH, ctx) {}
};

/// SuperHashSketch<Kmer, S>: S = f32 / f64, NoHashHasher (setsketchert.rs:211-336)
template <class Kmer, class S> class SuperHashSketch : public detail::SketcherImpl<Kmer, S, KMU_ALGO_SUPER> {
    static_assert(std::is_floating_point_v<S>, "SuperHashSketch: S is f32 or f64");

  public:
    explicit SuperHashSketch(const SeqSketcherParams &params, Context &ctx = Context::global())
        : detail::SketcherImpl<Kmer, S, KMU_ALGO_SUPER>(params, SketchAlgo::SUPER, KMU_HASHER_NOHASH, ctx) {}
};

/// OptDensHashSketch<Kmer, S>: one-permutation hashing + optimal densification, S = f32 / f64 (setsketchert.rs:343-463;
/// AA: aautils/setsketchert.rs:482-612)
template <class Kmer, class S> class OptDensHashSketch : public detail::SketcherImpl<Kmer, S, KMU_ALGO_OPTDENS> {
    static_assert(std::is_floating_point_v<S>, "OptDensHashSketch: S is f32 or f64");

  public:
    explicit OptDensHashSketch(const SeqSketcherParams &params, Context &ctx = Context::global())
        : detail::SketcherImpl<Kmer, S, KMU_ALGO_OPTDENS>(params, SketchAlgo::OPTDENS, KMU_HASHER_NOHASH, ctx) {}
};

/// RevOptDensHashSketch<Kmer, S>: reverse optimal densification, robust when the sketch is larger than the sequence
/// (setsketchert.rs:474-599; AA: aautils/setsketchert.rs:616-746)
template <class Kmer, class S> class RevOptDensHashSketch : public detail::SketcherImpl<Kmer, S, KMU_ALGO_REVOPTDENS> {
    static_assert(std::is_floating_point_v<S>, "RevOptDensHashSketch: S is f32 or f64");

  public:
    explicit RevOptDensHashSketch(const SeqSketcherParams &params, Context &ctx = Context::global())
        : detail::SketcherImpl<Kmer, S, KMU_ALGO_REVOPTDENS>(params, SketchAlgo::REVOPTDENS, KMU_HASHER_NOHASH, ctx) {}
};

/// probminhash::setsketcher::SetSketchParams as HyperLogLogSketch::new takes it (defaults of the crate, as recalled)
struct SetSketchParams {
    double b = 1.001;
    size_t m = 4096;
    double a = 20.;
    uint32_t q = 65534;
};
/// HllSeqsThreading (setsketchert.rs:600-636): how upstream splits a list of sequences over threads; kept for the signature
struct HllSeqsThreading {
    size_t nb_iter_thread = 4, thread_threshold = 10000000;
    size_t get_nb_iter_threads() const { return nb_iter_thread; }
    size_t get_thread_threshold() const { return thread_threshold; }
};

/// HyperLogLogSketch<Kmer, S>::new(&seq_params, hll_params, hll_threads) (setsketchert.rs:640-896; AA:
/// aautils/setsketchert.rs:780-1011): SetSketch registers, S = u16 / u32 / u64; the sketch has hll_params.m registers
template <class Kmer, class S> class HyperLogLogSketch : public SeqSketcherT<Kmer, S> {
    static_assert(std::is_same_v<S, uint16_t> || std::is_same_v<S, uint32_t> || std::is_same_v<S, uint64_t>, "S is u16, u32 or u64");

  public:
    using Seq = typename SeqSketcherT<Kmer, S>::Seq;
    HyperLogLogSketch(const SeqSketcherParams &seq_params, SetSketchParams hll_params, HllSeqsThreading hll_threads = {},
                      Context &ctx = Context::global())
        : params_(seq_params), hll_(hll_params), threads_(hll_threads), ctx_(ctx) {}
    size_t get_kmer_size() const override { return params_.get_kmer_size(); }
    size_t get_sketch_size() const override { return params_.get_sketch_size(); }
    SketchAlgo get_algo() const override { return SketchAlgo::HLL; }
    std::vector<std::vector<S>> sketch_compressedkmer(const std::vector<const Seq *> &vseq, FHash fhash) const override {
        return run(vseq, fhash, KMU_MODE_PER_SEQ);
    }
    std::vector<std::vector<S>> sketch_compressedkmer_seqs(const std::vector<const Seq *> &vseq, FHash fhash) const override {
        return run(vseq, fhash, KMU_MODE_ALL_SEQS);
    }
    std::vector<std::vector<S>> sketch_compressedkmer_seqs_groups(const std::vector<std::vector<const Seq *>> &groups,
                                                                  FHash fhash) const override {
        set_hll_params();
        return detail::run_sketch_groups<Kmer, S>(ctx_, groups, KMU_ALGO_HLL, params_.get_kmer_size(), hll_.m, sig, KMU_HASHER_NOHASH, fhash);
    }

  private:
    static constexpr int sig = std::is_same_v<S, uint16_t> ? KMU_SIG_U16 : std::is_same_v<S, uint32_t> ? KMU_SIG_U32 : KMU_SIG_U64;
    void set_hll_params() const {
        kmu_hll_params hp{hll_.b, hll_.a, hll_.q, 0};
        ctx_.check(kmu_set_hll_params(ctx_.raw(), &hp));
    }
    std::vector<std::vector<S>> run(const std::vector<const Seq *> &vseq, FHash fhash, int mode) const {
        set_hll_params();
        const detail::Batch b = detail::gather(vseq);
        kmu_sketch_params p = detail::sketch_params(KMU_ALGO_HLL, Kmer::kmu_type, params_.get_kmer_size(), hll_.m, sig,
                                                    KMU_HASHER_NOHASH, int(fhash), 0, mode, b.input_kind);
        const size_t rows = mode == KMU_MODE_ALL_SEQS ? 1 : b.n();
        std::vector<S> flat(rows * hll_.m);
        ctx_.check(kmu_sketch(ctx_.raw(), &p, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), nullptr, detail::ptr(flat), nullptr));
        return detail::split_rows(flat, rows, hll_.m);
    }
    SeqSketcherParams params_;
    SetSketchParams hll_;
    HllSeqsThreading threads_;
    Context &ctx_;
};

/// the `H: Hasher` parameter of SuperHash2Sketch
struct NoHashHasher { static constexpr int id = KMU_HASHER_NOHASH; };   // src/nohasher.rs
struct FnvHasher { static constexpr int id = KMU_HASHER_FNV1A; };       // fnv crate

/// SuperHash2Sketch<Kmer, S, H>: S = u32 / u64 (setsketchert.rs:904-1046)
template <class Kmer, class S, class H = NoHashHasher>
class SuperHash2Sketch : public detail::SketcherImpl<Kmer, S, KMU_ALGO_SUPER2> {
    static_assert(std::is_same_v<S, uint32_t> || std::is_same_v<S, uint64_t>, "SuperHash2Sketch: S is u32 or u64");

  public:
    explicit SuperHash2Sketch(const SeqSketcherParams &params, Context &ctx = Context::global())
        : detail::SketcherImpl<Kmer, S, KMU_ALGO_SUPER2>(params, SketchAlgo::SUPER2, H::id, ctx) {}
};

// =====================================================================================================================
// sketching: the older struct API, SeqSketcher (seqsketchjaccard.rs:117-415)
// =====================================================================================================================

class SeqSketcher {
  public:
    SeqSketcher(size_t kmer_size, size_t sketch_size, Context &ctx = Context::global())
        : kmer_size_(kmer_size), sketch_size_(sketch_size), ctx_(ctx) {}
    size_t get_kmer_size() const { return kmer_size_; }
    size_t get_sketch_size() const { return sketch_size_; }

    /// seqsketchjaccard.rs:211-260 (DNA), aautils/setsketchert.rs:114-150 (AA): Vec<Vec<Kmer::Val>>, row i <-> sequence i
    template <class Kmer, class Seq, class F>
    std::vector<std::vector<typename Kmer::Val>> sketch_probminhash3a(const std::vector<const Seq *> &vseq, F fhash) const {
        return detail::run_sketch<Kmer, typename Kmer::Val>(ctx_, detail::gather(vseq), KMU_ALGO_PROB3A, kmer_size_,
                                                            sketch_size_, KMU_HASHER_NOHASH, fhash, KMU_MODE_PER_SEQ);
    }
    /// the same on reads already gathered in the C-ABI form (what the FASTQ reader below returns)
    template <class Kmer, class F>
    std::vector<std::vector<typename Kmer::Val>> sketch_probminhash3a(const detail::Batch &reads, F fhash) const {
        return detail::run_sketch<Kmer, typename Kmer::Val>(ctx_, reads, KMU_ALGO_PROB3A, kmer_size_, sketch_size_,
                                                            KMU_HASHER_NOHASH, fhash, KMU_MODE_PER_SEQ);
    }
    /// ... and with the rows left row-major in a buffer the caller keeps from pack to pack (the tools' loop)
    template <class Kmer, class F>
    size_t sketch_probminhash3a(const detail::Batch &reads, F fhash, std::vector<typename Kmer::Val> &rows_out) const {
        return detail::run_sketch_flat<Kmer, typename Kmer::Val>(ctx_, reads, KMU_ALGO_PROB3A, kmer_size_, sketch_size_,
                                                                 KMU_HASHER_NOHASH, fhash, KMU_MODE_PER_SEQ, rows_out);
    }
    /// seqsketchjaccard.rs:272-319: ProbMinHash3 over the same weighted multiset
    template <class Kmer, class Seq, class F>
    std::vector<std::vector<typename Kmer::Val>> sketch_probminhash3(const std::vector<const Seq *> &vseq, F fhash) const {
        return detail::run_sketch<Kmer, typename Kmer::Val>(ctx_, detail::gather(vseq), KMU_ALGO_PROB3, kmer_size_,
                                                            sketch_size_, KMU_HASHER_NOHASH, fhash, KMU_MODE_PER_SEQ);
    }
    /// seqsketchjaccard.rs:328-380: SuperMinHash<S, Kmer::Val, fnv::FnvHasher>
    template <class Kmer, class S = double, class Seq, class F>
    std::vector<std::vector<S>> sketch_superminhash(const std::vector<const Seq *> &vseq, F fhash) const {
        return detail::run_sketch<Kmer, S>(ctx_, detail::gather(vseq), KMU_ALGO_SUPER, kmer_size_, sketch_size_,
                                           KMU_HASHER_FNV1A, fhash, KMU_MODE_PER_SEQ);
    }

    /// dump_json / reload_json (seqsketchjaccard.rs:142-201): {"kmer_size":..,"sketch_size":..}
    void dump_json(const std::string &filename) const {
        std::ofstream out(filename);
        if (!out) throw std::runtime_error("SeqSketcher dump failed");
        out << "{\"kmer_size\":" << kmer_size_ << ",\"sketch_size\":" << sketch_size_ << "}";
    }
    static SeqSketcher reload_json(const std::string &dirpath, Context &ctx = Context::global()) {
        const std::string text = detail::read_text_file(dirpath + "/sketchparams_dump.json");
        return SeqSketcher(std::stoul(detail::json_field(text, "kmer_size")), std::stoul(detail::json_field(text, "sketch_size")), ctx);
    }
    /// create_signature_dump: magic, sig_size = 4, sketch_size, kmer_size as four u32 (seqsketchjaccard.rs:385-414)
    std::ofstream create_signature_dump(const std::string &dumpfname) const {
        std::ofstream out(dumpfname, std::ios::binary);
        if (!out) throw std::runtime_error("create_signature_dump: cannot open " + dumpfname);
        const uint32_t head[4] = {MAGIC_SIG_DUMP, 4u, uint32_t(sketch_size_), uint32_t(kmer_size_)};
        out.write(reinterpret_cast<const char *>(head), sizeof head);
        return out;
    }
    /// dump_signatures_block_u32 (seqsketchjaccard.rs:572-583)
    static void dump_signatures_block_u32(const std::vector<std::vector<uint32_t>> &signatures, std::ostream &out) {
        for (const auto &sig : signatures) out.write(reinterpret_cast<const char *>(sig.data()), std::streamsize(4 * sig.size()));
    }
    static void dump_signatures_block_u32(const std::vector<uint32_t> &rows, size_t n_values, std::ostream &out) {
        out.write(reinterpret_cast<const char *>(rows.data()), std::streamsize(4 * n_values));
    }
    static constexpr uint32_t MAGIC_SIG_DUMP = 0xceabeadd;   // seqsketchjaccard.rs:570

  private:
    size_t kmer_size_, sketch_size_;
    Context &ctx_;
};

/// SigSketchFileReader::new / next (seqsketchjaccard.rs:586-712).  Upstream's `next` reads the bytes of a row but returns an
/// empty Vec (:690-708); this reader returns the row.
class SigSketchFileReader {
  public:
    explicit SigSketchFileReader(const std::string &fname) : in_(fname, std::ios::binary) {
        uint32_t head[4] = {0, 0, 0, 0};
        if (!in_) throw std::runtime_error("SigSketchFileReader could not open file " + fname);
        in_.read(reinterpret_cast<char *>(head), 16);
        if (in_.gcount() < 4) throw std::runtime_error("SigSketchFileReader could no read magic");
        if (head[0] != SeqSketcher::MAGIC_SIG_DUMP) throw std::runtime_error("file is not a dump of signature");
        if (in_.gcount() < 16) throw std::runtime_error("SigSketchFileReader could no read sketch_size");
        sig_size_ = head[1];
        sketch_size_ = head[2];
        kmer_size_ = uint8_t(head[3]);
        if (sig_size_ != 4) throw std::runtime_error("SigSketchFileReader , sig_size != 4 not yet implemented");
    }
    uint8_t get_kmer_size() const { return kmer_size_; }
    size_t get_signature_length() const { return sketch_size_; }
    size_t get_signature_size() const { return sig_size_; }
    /// the next signature, or nothing at the end of the file
    std::optional<std::vector<uint32_t>> next() {
        std::vector<uint32_t> row(sketch_size_);
        in_.read(reinterpret_cast<char *>(row.data()), std::streamsize(4 * sketch_size_));
        if (size_t(in_.gcount()) < 4 * sketch_size_) return std::nullopt;
        return row;
    }

  private:
    std::ifstream in_;
    size_t sig_size_ = 0, sketch_size_ = 0;
    uint8_t kmer_size_ = 0;
};

// =====================================================================================================================
// what callers do with signatures (seqsketchjaccard.rs:58-108, 423-495)
// =====================================================================================================================

namespace detail {
template <class D> uint32_t equal_slots(Context &ctx, const std::vector<D> &a, const std::vector<D> &b) {
    if (a.size() != b.size()) throw std::invalid_argument("signatures of different lengths");
    static_assert(sizeof(D) == 4 || sizeof(D) == 8, "signature element of 4 or 8 bytes");
    const uint32_t zero = 0;
    uint32_t out = 0;
    ctx.check(kmu_sig_equal_pairs(ctx.raw(), a.data(), 1, b.data(), 1, uint32_t(a.size()), sig_type_of<D>(), &zero, &zero, 1,
                                  KMU_MEM_HOST, &out));
    return out;
}
}  // namespace detail

/// compute_probminhash_jaccard (crate probminhash::jaccard): fraction of equal slots
template <class D> double compute_probminhash_jaccard(const std::vector<D> &siga, const std::vector<D> &sigb,
                                                      Context &ctx = Context::global()) {
    return double(detail::equal_slots(ctx, siga, sigb)) / double(siga.size());
}
/// get_jaccard_index_estimate of SuperMinHash sketches: likewise (seqsketchjaccard.rs:727-732)
template <class S> double compute_superminhash_jaccard(const std::vector<S> &hsketch, const std::vector<S> &other,
                                                       Context &ctx = Context::global()) {
    return double(detail::equal_slots(ctx, hsketch, other)) / double(hsketch.size());
}
/// probminhash_get_jaccard_objects -> (jp, Some(common objects) | None), seqsketchjaccard.rs:86-108
template <class D>
std::pair<double, std::optional<std::vector<D>>> probminhash_get_jaccard_objects(const std::vector<D> &siga,
                                                                                 const std::vector<D> &sigb,
                                                                                 Context &ctx = Context::global()) {
    const uint32_t inter = detail::equal_slots(ctx, siga, sigb);
    if (inter == 0) return {0.0, std::nullopt};
    std::vector<D> common;
    for (size_t i = 0; i < siga.size(); i++)
        if (siga[i] == sigb[i]) common.push_back(siga[i]);
    return {double(inter) / double(siga.size()), std::move(common)};
}

/// One entry of a neighbour list (the shape of hnsw_rs's `Neighbour`): row of the database, distance = (m - eq) / m
struct Neighbour {
    uint32_t idx;
    float distance;
};

/// kmu_sig_knn on row-major host signatures (`m` words per row): idx / eq lists of `k` entries per query row, ordered by
/// eq descending then row ascending; rows with group_q[i] == group_db[j] are never paired (null, null: no groups)
template <class D>
void sig_knn(const D *sig_q, size_t nq, const D *sig_db, size_t ndb, size_t m, size_t k, const uint32_t *group_q,
             const uint32_t *group_db, std::vector<uint32_t> &idx, std::vector<uint16_t> &eq, Context &ctx = Context::global()) {
    idx.assign(nq * k, KMU_KNN_NONE);
    eq.assign(nq * k, 0);
    ctx.check(kmu_sig_knn(ctx.raw(), nq ? sig_q : &detail::spare_element<D>, uint32_t(nq), ndb ? sig_db : &detail::spare_element<D>, uint32_t(ndb),
                          uint32_t(m), detail::sig_type_of<D>(), uint32_t(k), group_q, group_db, KMU_MEM_HOST, detail::ptr(idx), detail::ptr(eq)));
}

/// The exact answer to the query an HNSW index under DistHamming / DistBlockSketched approximates
/// (datasketcher.rs:137-192): per query row the k nearest database rows, nearest first; lists are shorter than k
/// when fewer candidates exist.
template <class D>
std::vector<std::vector<Neighbour>> nearest_neighbours(const std::vector<std::vector<D>> &sig_q,
                                                       const std::vector<std::vector<D>> &sig_db, size_t k,
                                                       const std::vector<uint32_t> *group_q = nullptr,
                                                       const std::vector<uint32_t> *group_db = nullptr,
                                                       Context &ctx = Context::global()) {
    const size_t m = sig_q.empty() ? (sig_db.empty() ? 1 : sig_db[0].size()) : sig_q[0].size();
    std::vector<D> fq, fdb;
    for (const auto &r : sig_q) {
        if (r.size() != m) throw std::invalid_argument("signatures of different lengths");
        fq.insert(fq.end(), r.begin(), r.end());
    }
    for (const auto &r : sig_db) {
        if (r.size() != m) throw std::invalid_argument("signatures of different lengths");
        fdb.insert(fdb.end(), r.begin(), r.end());
    }
    std::vector<uint32_t> idx;
    std::vector<uint16_t> eq;
    sig_knn(fq.data(), sig_q.size(), fdb.data(), sig_db.size(), m, k, group_q ? group_q->data() : nullptr,
            group_db ? group_db->data() : nullptr, idx, eq, ctx);
    std::vector<std::vector<Neighbour>> out(sig_q.size());
    for (size_t i = 0; i < sig_q.size(); i++)
        for (size_t l = 0; l < k && idx[i * k + l] != KMU_KNN_NONE; l++)
            out[i].push_back(Neighbour{idx[i * k + l], float(m - eq[i * k + l]) / float(m)});
    return out;
}

/// The neighbour file `datasketcher ... ann` writes beside a signature dump (this project's format, not hnsw_rs's graph
/// dump): magic u32, n_rows u64, k u32, sketch_size u32, n_rows x k u32 indices, n_rows x k u16 equal-slot counts
inline void write_neighbour_file(const std::string &fname, const std::vector<uint32_t> &idx, const std::vector<uint16_t> &eq,
                                 uint64_t n_rows, uint32_t k, uint32_t sketch_size) {
    std::ofstream out(fname, std::ios::binary);
    if (!out) throw std::runtime_error("write_neighbour_file: cannot open " + fname);
    const uint32_t magic = 0xceab0a22u;
    out.write(reinterpret_cast<const char *>(&magic), 4);
    out.write(reinterpret_cast<const char *>(&n_rows), 8);
    out.write(reinterpret_cast<const char *>(&k), 4);
    out.write(reinterpret_cast<const char *>(&sketch_size), 4);
    out.write(reinterpret_cast<const char *>(idx.data()), std::streamsize(n_rows * k * 4));
    out.write(reinterpret_cast<const char *>(eq.data()), std::streamsize(n_rows * k * 2));
}

/// jaccard_index_probminhash3a(seqa, vseqb, sketch_size, kmer_size, fhash) -> Vec<f64> (seqsketchjaccard.rs:423-495):
/// P-Jaccard estimate of seqa against every sequence of vseqb
template <class Kmer, class F>
std::vector<double> jaccard_index_probminhash3a(const Sequence &seqa, const std::vector<Sequence> &vseqb, size_t sketch_size,
                                                size_t kmer_size, F fhash, Context &ctx = Context::global()) {
    std::vector<const Sequence *> all{&seqa};
    for (const Sequence &s : vseqb) all.push_back(&s);
    auto sigs = SeqSketcher(kmer_size, sketch_size, ctx).sketch_probminhash3a<Kmer>(all, fhash);
    std::vector<double> jac;
    for (size_t i = 1; i < sigs.size(); i++) jac.push_back(compute_probminhash_jaccard(sigs[0], sigs[i], ctx));
    return jac;
}

// =====================================================================================================================
// block sketching (seqblocksketch.rs)
// =====================================================================================================================

struct BlockSketched {   // seqblocksketch.rs:38-66
    uint32_t numseq;
    uint32_t numblock;
    std::vector<uint32_t> sketch;
    void dump(std::ostream &out) const {
        out.write(reinterpret_cast<const char *>(&numseq), 4);
        out.write(reinterpret_cast<const char *>(&numblock), 4);
        out.write(reinterpret_cast<const char *>(sketch.data()), std::streamsize(4 * sketch.size()));
    }
};

struct BlockSketchedSeq {   // seqblocksketch.rs:73-76
    uint32_t numseq;
    std::vector<BlockSketched> sketch;
};

/// Distance<BlockSketched>: 1 between blocks of one sequence, else the fraction of differing slots (seqblocksketch.rs:419-431)
class DistBlockSketched {
  public:
    explicit DistBlockSketched(Context &ctx = Context::global()) : ctx_(ctx) {}
    float eval(const BlockSketched &va, const BlockSketched &vb) const {
        if (va.numseq == vb.numseq) return 1.f;
        const uint32_t eq = detail::equal_slots(ctx_, va.sketch, vb.sketch);
        return float(va.sketch.size() - eq) / float(va.sketch.size());
    }

  private:
    Context &ctx_;
};

/// BlockSeqSketcher{block_size, kmer_size, sketch_size}: Kmer32bit / u32 only (seqblocksketch.rs:79-227)
class BlockSeqSketcher {
  public:
    BlockSeqSketcher(size_t block_size, size_t kmer_size, size_t sketch_size, Context &ctx = Context::global())
        : block_size_(block_size), kmer_size_(kmer_size), sketch_size_(sketch_size), ctx_(ctx) {}

    /// blocksketch_sequence(numseq, seq, fhash): seqblocksketch.rs:97-149
    BlockSketchedSeq blocksketch_sequence(size_t numseq, const Sequence &seq, FHash fhash) const {
        return std::move(blocksketch_sequences(numseq, {&seq}, fhash)[0]);
    }
    /// blocksketch_sequences(numfirst, seqs, fhash): sequence i gets numseq = numfirst + i (seqblocksketch.rs:152-167)
    std::vector<BlockSketchedSeq> blocksketch_sequences(size_t numfirst, const std::vector<const Sequence *> &seqs,
                                                        FHash fhash) const {
        return blocksketch_sequences(numfirst, detail::gather(seqs), fhash);
    }
    std::vector<BlockSketchedSeq> blocksketch_sequences(size_t numfirst, const detail::Batch &b, FHash fhash) const {
        std::vector<uint64_t> rows(b.n() + 1);
        ctx_.check(kmu_block_layout(b.offsets.data(), b.n(), uint32_t(block_size_), rows.data()));
        kmu_sketch_params p = detail::sketch_params(KMU_ALGO_PROB3A, KMU_KMER32BIT, kmer_size_, sketch_size_, KMU_SIG_U32,
                                                    KMU_HASHER_NOHASH, int(fhash), int(block_size_), KMU_MODE_PER_SEQ,
                                                    b.input_kind);
        p.mem = b.mem();
        std::vector<uint32_t> flat(std::max<uint64_t>(rows.back(), 1) * sketch_size_);
        if (b.on_device()) {
            DeviceBuffer d_rows(ctx_, rows.size() * 8), d_sig(ctx_, flat.size() * 4);
            d_rows.upload(rows.data(), rows.size() * 8);
            ctx_.check(kmu_sketch(ctx_.raw(), &p, b.dev_bytes, b.dev_offsets, nullptr, b.n(), d_rows.as<uint64_t>(), d_sig.data(),
                                  nullptr));
            d_sig.download(flat.data(), flat.size() * 4);
        } else {
            ctx_.check(kmu_sketch(ctx_.raw(), &p, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), rows.data(),
                                  flat.data(), nullptr));
        }
        std::vector<BlockSketchedSeq> out(b.n());
        for (uint32_t i = 0; i < b.n(); i++) {
            out[i].numseq = uint32_t(numfirst + i);
            for (uint64_t r = rows[i]; r < rows[i + 1]; r++)
                out[i].sketch.push_back(BlockSketched{uint32_t(numfirst + i), uint32_t(r - rows[i]),
                                                      {flat.begin() + r * sketch_size_, flat.begin() + (r + 1) * sketch_size_}});
        }
        return out;
    }

    /// create_signature_dump: magic u32, sig_size as ONE byte, sketch_size, kmer_size, block_size u32 = 17 bytes
    /// (seqblocksketch.rs:172-226)
    std::ofstream create_signature_dump(const std::string &dumpfname) const {
        std::ofstream out(dumpfname, std::ios::binary);
        if (!out) throw std::runtime_error("create_signature_dump: cannot open " + dumpfname);
        const uint32_t magic = MAGIC_BLOCKSIG_DUMP, tail[3] = {uint32_t(sketch_size_), uint32_t(kmer_size_), uint32_t(block_size_)};
        const uint8_t sig_size = 4;
        out.write(reinterpret_cast<const char *>(&magic), 4);
        out.write(reinterpret_cast<const char *>(&sig_size), 1);
        out.write(reinterpret_cast<const char *>(tail), sizeof tail);
        return out;
    }
    /// dump_blocks: per sequence numseq u32, nbblock u32, then BlockSketched::dump of every block
    static void dump_blocks(std::ostream &out, const std::vector<BlockSketchedSeq> &seqs) {
        for (const BlockSketchedSeq &s : seqs) {
            const uint32_t nb = uint32_t(s.sketch.size());
            out.write(reinterpret_cast<const char *>(&s.numseq), 4);
            out.write(reinterpret_cast<const char *>(&nb), 4);
            for (const BlockSketched &b : s.sketch) b.dump(out);
        }
    }
    static constexpr uint32_t MAGIC_BLOCKSIG_DUMP = 0xceabbadd;   // seqblocksketch.rs:33

  private:
    size_t block_size_, kmer_size_, sketch_size_;
    Context &ctx_;
};

// =====================================================================================================================
// bottom-k with multiplicities (minhash.rs)
// =====================================================================================================================

struct InvHashCount {   // hashed.rs: (hash, count)
    uint64_t hashed;
    uint16_t count;
};

struct MinHashDist {   // minhash.rs:134-190: containment, jaccard, common, total
    double containment, jaccard;
    uint64_t common, total;
};

namespace detail {
/// kmu_minhash_distance_pairs on the one pair of two padded sketches of one length
inline MinHashDist minhash_pair(Context &ctx, const std::vector<uint64_t> &ha, const std::vector<uint64_t> &hb) {
    const uint32_t zero = 0;
    uint32_t out[3] = {0, 0, 0};
    ctx.check(kmu_minhash_distance_pairs(ctx.raw(), ha.data(), 1, hb.data(), 1, uint32_t(ha.size()), &zero, &zero, 1, KMU_MEM_HOST, out));
    return MinHashDist{double(out[0]) / double(out[2]), double(out[0]) / double(out[1]), out[0], out[1]};
}
}  // namespace detail

/// MinInvHashCountKmer<Kmer, H>: the `size` smallest int64_hash(value) with u16 multiplicities (minhash.rs:194-290)
template <class Kmer> class MinInvHashCountKmer {
  public:
    explicit MinInvHashCountKmer(size_t size, Context &ctx = Context::global()) : size_(size), ctx_(ctx) {}
    /// sketch_kmer_slice: add k-mers (their compressed values)
    void sketch_kmer_slice(const std::vector<Kmer> &kmers) {
        for (const Kmer &k : kmers) pending_.push_back(typename Kmer::Val(k.get_compressed_value()));
    }
    /// get_sketchcount: ascending hashes (minhash.rs:275-289)
    std::vector<InvHashCount> get_sketchcount() const {
        using Val = typename Kmer::Val;
        std::vector<Val> vals = pending_;
        if (vals.empty()) return {};
        const uint64_t off[2] = {0, vals.size()};
        kmu_sketch_params p = detail::sketch_params(KMU_ALGO_BOTTOMK, Kmer::kmu_type, 0, size_, KMU_SIG_U64,
                                                    KMU_HASHER_INT64HASH, KMU_FHASH_IDENTITY_RAW, 0, KMU_MODE_PER_SEQ,
                                                    KMU_INPUT_ASCII);
        std::vector<uint64_t> h(size_);
        std::vector<uint32_t> c(size_);
        ctx_.check(kmu_sketch_hashed(ctx_.raw(), &p, vals.data(), off, 1, h.data(), c.data()));
        std::vector<InvHashCount> out;
        for (size_t i = 0; i < size_ && h[i] != UINT64_MAX; i++) out.push_back({h[i], uint16_t(c[i])});
        return out;
    }
    std::vector<uint64_t> get_hashes_padded() const {
        std::vector<uint64_t> h(size_, UINT64_MAX);
        auto sc = get_sketchcount();
        for (size_t i = 0; i < sc.size(); i++) h[i] = sc[i].hashed;
        return h;
    }
    size_t size() const { return size_; }

  private:
    size_t size_;
    Context &ctx_;
    std::vector<typename Kmer::Val> pending_;
};

/// minhash_distance / mininvhash_distance of two bottom-k sketches (minhash.rs:134-190, 295-340)
template <class Kmer>
MinHashDist mininvhash_distance(const MinInvHashCountKmer<Kmer> &a, const MinInvHashCountKmer<Kmer> &b,
                                Context &ctx = Context::global()) {
    if (a.size() != b.size()) throw std::invalid_argument("sketches of different sizes");
    return detail::minhash_pair(ctx, a.get_hashes_padded(), b.get_hashes_padded());
}

/// HashCount<u32> of seqminhash.rs: a kept hash and its multiplicity
struct HashCount {
    uint64_t hashed;
    uint16_t count;
};

namespace detail {
inline int range_kmer_type(size_t kmer_size) {
    if (kmer_size == 16) return KMU_KMER16B32BIT;
    if (kmer_size >= 9 && kmer_size <= 15) return KMU_KMER32BIT;
    throw std::invalid_argument("sketch_seqrange: unimplemented kmer_size");   // upstream panics (seqminhash.rs:53, :111)
}
/// the bases [start, end) of a packed sequence as a one-sequence ASCII batch (KmerSeqIterator::set_range keeps the k-mers
/// that lie inside the range)
inline Batch range_batch(const Sequence &seq, size_t start, size_t end) {
    if (end <= start || end > seq.size()) throw std::invalid_argument("bad range");   // set_range -> Err -> panic("bad range")
    Batch b;
    b.bytes.resize(end - start + 16, 0);
    for (size_t i = start; i < end; i++) b.bytes[i - start] = Alphabet2b::decode(seq.get_base(i));
    b.offsets = {0, end - start};
    return b;
}
}  // namespace detail

/// sketch_seqrange_superminhash(seq, range, kmer_size, sketch_size) -> Vec<f64> (seqminhash.rs:19-62):
/// SuperMinHash<f64, u32, NoHashHasher> over int32_hash(canonical k-mer); kmer_size 16 (Kmer16b32bit) or 9..15 (Kmer32bit)
inline std::vector<double> sketch_seqrange_superminhash(const Sequence &seq, std::pair<size_t, size_t> range, size_t kmer_size,
                                                        size_t sketch_size, Context &ctx = Context::global()) {
    kmu_sketch_params p = detail::sketch_params(KMU_ALGO_SUPER, detail::range_kmer_type(kmer_size), kmer_size, sketch_size,
                                                KMU_SIG_F64, KMU_HASHER_NOHASH, KMU_FHASH_CANON_INVHASH, 0, KMU_MODE_PER_SEQ,
                                                KMU_INPUT_ASCII);
    detail::Batch b = detail::range_batch(seq, range.first, range.second);
    std::vector<double> sig(sketch_size);
    ctx.check(kmu_sketch(ctx.raw(), &p, b.bytes.data(), b.offsets.data(), nullptr, 1, nullptr, sig.data(), nullptr));
    return sig;
}

/// sketch_seqrange_minhash(...) -> Vec<HashCount<u32>> (seqminhash.rs:65-119): MinHashCount<u32, NoHashHasher> over the same
/// values; returned ascending by hash (upstream: heap order)
inline std::vector<HashCount> sketch_seqrange_minhash(const Sequence &seq, std::pair<size_t, size_t> range, size_t kmer_size,
                                                      size_t sketch_size, Context &ctx = Context::global()) {
    kmu_sketch_params p = detail::sketch_params(KMU_ALGO_BOTTOMK, detail::range_kmer_type(kmer_size), kmer_size, sketch_size,
                                                KMU_SIG_U64, KMU_HASHER_NOHASH, KMU_FHASH_CANON_INVHASH, 0, KMU_MODE_PER_SEQ,
                                                KMU_INPUT_ASCII);
    detail::Batch b = detail::range_batch(seq, range.first, range.second);
    std::vector<uint64_t> h(sketch_size);
    std::vector<uint32_t> c(sketch_size);
    ctx.check(kmu_sketch(ctx.raw(), &p, b.bytes.data(), b.offsets.data(), nullptr, 1, nullptr, h.data(), c.data()));
    std::vector<HashCount> out;
    for (size_t i = 0; i < sketch_size && h[i] != UINT64_MAX; i++) out.push_back({h[i], uint16_t(c[i])});
    return out;
}

/// minhash_distance(&sk1, &sk2) -> MinHashDist (minhash.rs:134-190)
inline MinHashDist minhash_distance(const std::vector<HashCount> &sk1, const std::vector<HashCount> &sk2,
                                    Context &ctx = Context::global()) {
    const size_t m = std::max(sk1.size(), sk2.size());
    std::vector<uint64_t> ha(std::max<size_t>(m, 1), UINT64_MAX), hb(std::max<size_t>(m, 1), UINT64_MAX);
    for (size_t i = 0; i < sk1.size(); i++) ha[i] = sk1[i].hashed;
    for (size_t i = 0; i < sk2.size(); i++) hb[i] = sk2[i].hashed;
    return detail::minhash_pair(ctx, ha, hb);
}

// =====================================================================================================================
// read anchors (anchor.rs, without its redis storage)
// =====================================================================================================================

/// AnchorsGeneratorParameters::new(fasta_name, window, nbkmer, kmer_size, overlap) (anchor.rs:29-78)
class AnchorsGeneratorParameters {
  public:
    AnchorsGeneratorParameters(std::string fasta_name, uint32_t window, uint32_t nbkmer, uint16_t kmer_size, uint32_t overlap)
        : fasta_name_(std::move(fasta_name)), window_(window), nbkmer_(nbkmer), overlap_(overlap), kmer_size_(kmer_size) {}
    const std::string &get_fasta_name() const { return fasta_name_; }
    uint32_t get_window() const { return window_; }
    uint32_t get_nbkmer() const { return nbkmer_; }
    uint16_t get_kmer_size() const { return kmer_size_; }
    uint32_t get_overlap() const { return overlap_; }

  private:
    std::string fasta_name_;
    uint32_t window_, nbkmer_, overlap_;
    uint16_t kmer_size_;
};

/// SliceAnchor<Kmer> (anchor.rs:97-105): one window of a read -- the read, the first base of the slice, and its (hash, count)
/// pairs ascending by hash (empty for a slice that holds no k-mer)
template <class Kmer> struct SliceAnchor {
    uint32_t readnum;
    uint32_t slicepos;
    std::vector<InvHashCount> minhash;
    /// the slice's key in the inverse index (get_minhash_key_for_redis, anchor.rs:149-158)
    uint64_t get_minhash_key() const { return minhash.at(0).hashed; }
};

/// ReadAnchors<Kmer> (anchor.rs:265-329): the slices of one read
template <class Kmer> struct ReadAnchors {
    uint32_t readnum;
    std::vector<SliceAnchor<Kmer>> anchors;
    size_t get_nb_slice() const { return anchors.size(); }
};

/// ReadAnchors::generate_anchors for every read of a batch in one library call (kmu_read_anchors): read i is numbered
/// numfirst + i.  The defaults are the reference's MinInvHashCountKmer (forward k-mers, int64_hash of the compressed value,
/// u8 counts); FHash::canon_value gives strand-independent anchors.
template <class Kmer>
std::vector<ReadAnchors<Kmer>> gen_read_anchors(const AnchorsGeneratorParameters &params, size_t numfirst, const detail::Batch &batch,
                                                FHash fhash = FHash::value_masked, int hasher = KMU_HASHER_INT64HASH,
                                                Context &ctx = Context::global()) {
    const detail::Batch b = detail::unpacked(batch);
    const size_t m = params.get_nbkmer();
    std::vector<uint64_t> rows(b.n() + 1);
    ctx.check(kmu_anchor_layout(b.offsets.data(), b.n(), params.get_window(), params.get_overlap(), rows.data()));
    kmu_sketch_params p = detail::sketch_params(KMU_ALGO_BOTTOMK, Kmer::kmu_type, params.get_kmer_size(), m, KMU_SIG_U64, hasher,
                                                int(fhash), 0, KMU_MODE_PER_SEQ, KMU_INPUT_ASCII);
    p.mem = b.mem();
    const size_t n_rows = size_t(std::max<uint64_t>(rows.back(), 1));
    std::vector<uint64_t> h(n_rows * m);
    std::vector<uint32_t> c(n_rows * m), n(n_rows);
    if (b.on_device()) {
        DeviceBuffer d_rows(ctx, rows.size() * 8), d_h(ctx, h.size() * 8), d_c(ctx, c.size() * 4), d_n(ctx, n.size() * 4);
        d_rows.upload(rows.data(), rows.size() * 8);
        ctx.check(kmu_read_anchors(ctx.raw(), &p, b.dev_bytes, b.dev_offsets, b.n(), params.get_window(), params.get_overlap(),
                                   d_rows.as<uint64_t>(), d_h.as<uint64_t>(), d_c.as<uint32_t>(), d_n.as<uint32_t>()));
        if (rows.back()) {
            d_h.download(h.data(), h.size() * 8);
            d_c.download(c.data(), c.size() * 4);
            d_n.download(n.data(), n.size() * 4);
        }
    } else {
        ctx.check(kmu_read_anchors(ctx.raw(), &p, b.bytes.data(), b.offsets.data(), b.n(), params.get_window(), params.get_overlap(),
                                   rows.data(), h.data(), c.data(), n.data()));
    }
    const uint32_t stride = params.get_window() - params.get_overlap();
    std::vector<ReadAnchors<Kmer>> out(b.n());
    for (uint32_t i = 0; i < b.n(); i++) {
        out[i].readnum = uint32_t(numfirst + i);
        for (uint64_t r = rows[i]; r < rows[i + 1]; r++) {
            SliceAnchor<Kmer> s{uint32_t(numfirst + i), uint32_t((r - rows[i]) * stride), {}};
            for (uint32_t t = 0; t < n[r]; t++) s.minhash.push_back({h[r * m + t], uint16_t(c[r * m + t])});
            out[i].anchors.push_back(std::move(s));
        }
    }
    return out;
}
template <class Kmer>
std::vector<ReadAnchors<Kmer>> gen_read_anchors(const AnchorsGeneratorParameters &params, size_t numfirst,
                                                const std::vector<const Sequence *> &seqs, FHash fhash = FHash::value_masked,
                                                int hasher = KMU_HASHER_INT64HASH, Context &ctx = Context::global()) {
    return gen_read_anchors<Kmer>(params, numfirst, detail::gather(seqs), fhash, hasher, ctx);
}

/// one hit of match_read_anchors: slice a (readnum_a, slicepos_a) and slice b of another read share one of their smallest hashes;
/// common / total are mininvhash_distance's counts for (a first, b second)
struct AnchorMatch {
    uint32_t readnum_a, slicepos_a, readnum_b, slicepos_b, common, total;
    bool operator==(const AnchorMatch &o) const {
        return readnum_a == o.readnum_a && slicepos_a == o.slicepos_a && readnum_b == o.readnum_b && slicepos_b == o.slicepos_b &&
               common == o.common && total == o.total;
    }
};

namespace detail {
/// two_calls of anchor matching: `call(pairs_out, dist_out, cap, n_out)`; `pairs` holds 2 and `dist` 3 values for each pair
template <class Call> uint64_t match_calls(Context &ctx, std::vector<uint32_t> &pairs, std::vector<uint32_t> &dist, Call call) {
    return two_calls(
        ctx, false, [&](uint64_t total) { pairs.assign(size_t(total) * 2, 0), dist.assign(size_t(total) * 3, 0); },
        [&](bool write, uint64_t cap, uint64_t *total) { return call(write ? pairs.data() : nullptr, write ? dist.data() : nullptr, cap, total); });
}
}  // namespace detail

/// kmu_anchor_index: bottom-k rows (ndb x m, ascending, UINT64_MAX padding), their n_keys smallest hashes sorted into buckets and
/// optionally the group of every row, kept on the device -- the inverse index of `redis_dump` (anchor.rs:187-197) as an object that
/// is built once and matched against by any number of query batches.  It copies what it is given and must not outlive its context.
class AnchorIndex {
  public:
    /// `group_db` empty: no groups (then match takes none either)
    AnchorIndex(const std::vector<uint64_t> &hashes_db, uint32_t ndb, uint32_t m, uint32_t n_keys = 1,
                const std::vector<uint32_t> &group_db = {}, Context &ctx = Context::global())
        : ctx_(&ctx), m_(m) {
        if (hashes_db.size() < size_t(ndb) * m || (!group_db.empty() && group_db.size() < ndb))
            throw std::invalid_argument("AnchorIndex: hashes_db holds ndb x m hashes, group_db ndb groups");
        ctx.check(kmu_anchor_index_create(ctx.raw(), ndb ? hashes_db.data() : &detail::spare_element<uint64_t>, ndb, m, n_keys, detail::opt(group_db),
                                          KMU_MEM_HOST, &ix_));
    }
    ~AnchorIndex() { kmu_anchor_index_destroy(ix_); }
    AnchorIndex(AnchorIndex &&o) noexcept : ctx_(o.ctx_), ix_(o.ix_), m_(o.m_) { o.ix_ = nullptr; }
    AnchorIndex(const AnchorIndex &) = delete;
    AnchorIndex &operator=(const AnchorIndex &) = delete;

    kmu_anchor_index *raw() const { return ix_; }
    kmu_anchor_index_info_t info() const {
        kmu_anchor_index_info_t t{};
        ctx_->check(kmu_anchor_index_info(ix_, &t));
        return t;
    }
    /// hist[c] = the distinct keys that c database rows carry; the last bin collects every c >= n_bins - 1
    std::vector<uint64_t> occupancy(uint32_t n_bins) const {
        std::vector<uint64_t> hist(n_bins, 0);
        ctx_->check(kmu_anchor_index_occupancy(ix_, hist.data(), n_bins, KMU_MEM_HOST));
        return hist;
    }
    /// kmu_anchor_index_match of nq query rows (nq x m; `group_q` empty iff the index has no groups): `pairs` gets (a, b) and
    /// `dist` (common, total, i) of every pair, ordered by a, shared hash, b.  max_occ > 0: hashes that are keys of more than
    /// max_occ database rows seed no pair; 0: the result of kmu_anchor_match.  Returns the number of pairs.
    uint64_t match(const std::vector<uint64_t> &hashes_q, uint32_t nq, const std::vector<uint32_t> &group_q, uint32_t min_common,
                   uint32_t max_occ, std::vector<uint32_t> &pairs, std::vector<uint32_t> &dist) const {
        if (hashes_q.size() < size_t(nq) * m_ || (!group_q.empty() && group_q.size() < nq))
            throw std::invalid_argument("AnchorIndex::match: hashes_q holds nq x m hashes, group_q nq groups");
        const uint64_t *q = nq ? hashes_q.data() : &detail::spare_element<uint64_t>;
        const uint32_t *g = detail::opt(group_q);
        return detail::match_calls(*ctx_, pairs, dist, [&](uint32_t *p, uint32_t *d, uint64_t cap, uint64_t *n) {
            return kmu_anchor_index_match(ix_, q, nq, g, min_common, max_occ, KMU_MEM_HOST, p, d, cap, n);
        });
    }

  private:
    Context *ctx_;
    kmu_anchor_index *ix_ = nullptr;
    uint32_t m_;
};

namespace detail {
/// the slices of `reads` as bottom-k rows of m hashes (UINT64_MAX padding; one padding row where there is no slice), and the read
/// of every slice as its group
template <class Kmer> std::vector<uint64_t> anchor_rows(const std::vector<ReadAnchors<Kmer>> &reads, size_t m, std::vector<uint32_t> &group) {
    for (size_t i = 0; i < reads.size(); i++) group.insert(group.end(), reads[i].anchors.size(), uint32_t(i));
    std::vector<uint64_t> h(std::max<size_t>(group.size(), 1) * m, UINT64_MAX);
    size_t r = 0;
    for (const ReadAnchors<Kmer> &ra : reads)
        for (const SliceAnchor<Kmer> &s : ra.anchors) {
            for (size_t t = 0; t < s.minhash.size() && t < m; t++) h[r * m + t] = s.minhash[t].hashed;
            r++;
        }
    return h;
}

/// the window pairs of `rows` bottom-k rows against themselves, slices of one group never paired: kmu_anchor_match, or with a repeat
/// mask (max_occ > 0) an AnchorIndex of the rows
inline void anchor_self_join(const std::vector<uint64_t> &h, uint32_t rows, uint32_t m, uint32_t n_keys, uint32_t min_common,
                             const std::vector<uint32_t> &group, uint32_t max_occ, Context &ctx, std::vector<uint32_t> &pairs,
                             std::vector<uint32_t> &dist) {
    if (max_occ) {
        if (rows) AnchorIndex(h, rows, m, n_keys, group, ctx).match(h, rows, group, min_common, max_occ, pairs, dist);
        else { pairs.clear(); dist.clear(); }
        return;
    }
    match_calls(ctx, pairs, dist, [&](uint32_t *p, uint32_t *d, uint64_t cap, uint64_t *n) {
        return kmu_anchor_match(ctx.raw(), h.data(), rows, h.data(), rows, m, n_keys, min_common, group.data(), group.data(), KMU_MEM_HOST,
                                p, d, cap, n);
    });
}
}  // namespace detail

/// What looking every slice up in the inverse index of `redis_dump` (anchor.rs:187-197; n_keys = 1 is its MINHASH_1) finds among the
/// slices of `reads` (the result of gen_read_anchors), with mininvhash_distance for each hit: kmu_anchor_match as a self-join with
/// group = read.  Slices of one read are never paired; hits with common < min_common are dropped; (a, b) and (b, a) are both
/// reported.  Order: slice a in the order of `reads`, then the shared hash, then slice b.  max_occ > 0: hashes that are keys of more
/// than max_occ slices seed no pair (an AnchorIndex of the slices).
template <class Kmer>
std::vector<AnchorMatch> match_read_anchors(const std::vector<ReadAnchors<Kmer>> &reads, const AnchorsGeneratorParameters &params,
                                            uint32_t n_keys = 1, uint32_t min_common = 1, uint32_t max_occ = 0,
                                            Context &ctx = Context::global()) {
    const size_t m = params.get_nbkmer();
    std::vector<const SliceAnchor<Kmer> *> slices;
    for (const ReadAnchors<Kmer> &ra : reads)
        for (const SliceAnchor<Kmer> &s : ra.anchors) slices.push_back(&s);
    std::vector<uint32_t> group;
    const std::vector<uint64_t> h = detail::anchor_rows(reads, m, group);
    const uint32_t rows = uint32_t(slices.size());
    std::vector<uint32_t> pairs, dist;
    detail::anchor_self_join(h, rows, uint32_t(m), n_keys, min_common, group, max_occ, ctx, pairs, dist);
    std::vector<AnchorMatch> out(pairs.size() / 2);
    for (size_t p = 0; p < out.size(); p++) {
        const SliceAnchor<Kmer> &a = *slices[pairs[2 * p]], &b = *slices[pairs[2 * p + 1]];
        out[p] = AnchorMatch{a.readnum, a.slicepos, b.readnum, b.slicepos, dist[3 * p], dist[3 * p + 1]};
    }
    return out;
}

/// kmu_anchor_overlaps on host arrays: the read pairs behind the window pairs `pairs` (2 per pair, rows of the two sides) of
/// kmu_anchor_match, one kmu_overlap each (include/kmu.h has the rules).  `dist` (3 per pair) weighs a pair by its common; empty:
/// every pair weighs 1.  row_offsets_*: the arrays of kmu_anchor_layout of the two sides.  upper: only read_a < read_b.
inline std::vector<kmu_overlap> anchor_overlaps(const std::vector<uint32_t> &pairs, const std::vector<uint32_t> &dist,
                                                const std::vector<uint64_t> &row_offsets_q, const std::vector<uint64_t> &row_offsets_db,
                                                uint32_t strands = 2, uint32_t band = 1, uint32_t min_score = 1, bool upper = false,
                                                Context &ctx = Context::global()) {
    if (row_offsets_q.empty() || row_offsets_db.empty()) throw std::invalid_argument("anchor_overlaps: row offsets hold n_reads + 1 entries");
    if (!dist.empty() && dist.size() / 3 != pairs.size() / 2) throw std::invalid_argument("anchor_overlaps: dist holds 3 values per pair");
    const uint64_t n_pairs = pairs.size() / 2;
    const uint32_t flags = upper ? KMU_OVL_UPPER : 0u, nq = uint32_t(row_offsets_q.size() - 1), ndb = uint32_t(row_offsets_db.size() - 1);
    const uint32_t *pp = n_pairs ? pairs.data() : &detail::spare_element<uint32_t>;
    std::vector<kmu_overlap> out;
    detail::two_calls(
        ctx, false, [&](uint64_t total) { out.resize(size_t(total)); },
        [&](bool, uint64_t cap, uint64_t *total) {
            return kmu_anchor_overlaps(ctx.raw(), pp, detail::opt(dist), n_pairs, row_offsets_q.data(), nq, row_offsets_db.data(), ndb, strands, band,
                                       min_score, flags, KMU_MEM_HOST, detail::opt(out), cap, total);
        });
    return out;
}

/// one read pair of read_overlaps: read b lies on `strand` of read a (0: the same, 1: the opposite) at `offset` bases -- the first
/// diagonal of the winning band times the stride; the difference of the slice positions on strand 0, their sum on strand 1 -- with
/// the band's weight, its number of matched slices, and the first and last slicepos of read a among them
struct Overlap {
    uint32_t readnum_a, readnum_b, strand;
    int64_t offset;
    uint32_t score, votes, slicepos_a_first, slicepos_a_last;
    bool operator==(const Overlap &o) const {
        return readnum_a == o.readnum_a && readnum_b == o.readnum_b && strand == o.strand && offset == o.offset && score == o.score &&
               votes == o.votes && slicepos_a_first == o.slicepos_a_first && slicepos_a_last == o.slicepos_a_last;
    }
};

namespace detail {
/// the kmu_overlap records of `reads` against themselves (each read pair once, read indices into `reads`): the front of
/// read_overlaps and read_clusters
template <class Kmer>
std::vector<kmu_overlap> read_overlap_records(const std::vector<ReadAnchors<Kmer>> &reads, const AnchorsGeneratorParameters &params,
                                              uint32_t n_keys, uint32_t min_common, uint32_t strands, uint32_t band, uint32_t min_score,
                                              uint32_t max_occ, Context &ctx) {
    const size_t m = params.get_nbkmer();
    std::vector<uint64_t> row_offsets(reads.size() + 1, 0);
    for (size_t i = 0; i < reads.size(); i++) row_offsets[i + 1] = row_offsets[i] + reads[i].anchors.size();
    std::vector<uint32_t> group;
    const std::vector<uint64_t> h = anchor_rows(reads, m, group);
    const uint32_t rows = uint32_t(group.size());
    std::vector<uint32_t> pairs, dist;
    anchor_self_join(h, rows, uint32_t(m), n_keys, min_common, group, max_occ, ctx, pairs, dist);
    return anchor_overlaps(pairs, dist, row_offsets, row_offsets, strands, band, min_score, true, ctx);
}
}  // namespace detail

/// Which of `reads` (the result of gen_read_anchors) overlap: the self-join of match_read_anchors, then kmu_anchor_overlaps with
/// the common of every matched pair of slices as its weight, each read pair once (a in front of b in `reads`).  strands = 2 is for
/// anchors made with FHash::canon_value.  Order: read a, then read b, in the order of `reads`.  max_occ: the repeat mask of
/// match_read_anchors.
template <class Kmer>
std::vector<Overlap> read_overlaps(const std::vector<ReadAnchors<Kmer>> &reads, const AnchorsGeneratorParameters &params,
                                   uint32_t n_keys = 1, uint32_t min_common = 1, uint32_t strands = 2, uint32_t band = 1,
                                   uint32_t min_score = 2, uint32_t max_occ = 0, Context &ctx = Context::global()) {
    const int64_t stride = int64_t(params.get_window()) - int64_t(params.get_overlap());
    std::vector<Overlap> out;
    for (const kmu_overlap &o : detail::read_overlap_records(reads, params, n_keys, min_common, strands, band, min_score, max_occ, ctx))
        out.push_back(Overlap{reads[o.read_a].readnum, reads[o.read_b].readnum, o.strand, int64_t(o.diag) * stride, o.score, o.votes,
                              uint32_t(o.slice_a_min * stride), uint32_t(o.slice_a_max * stride)});
    return out;
}

/// what kmu_components gives for n nodes: label[v] the smallest node of v's component, cluster[v] its dense number (clusters in
/// the order of their smallest node), size[c] for c < n_components, members the nodes by (cluster, node)
struct Components {
    std::vector<uint32_t> label, cluster, size, members;
    uint32_t n_components = 0;
};

namespace detail {
template <class Call> Components components_call(Context &ctx, uint32_t n_nodes, Call call) {
    Components c;
    c.label.assign(n_nodes, 0);
    c.cluster.assign(n_nodes, 0);
    c.size.assign(n_nodes, 0);
    c.members.assign(n_nodes, 0);
    ctx.check(call(ptr(c.label), ptr(c.cluster), ptr(c.size), ptr(c.members), &c.n_components));
    c.size.resize(c.n_components);
    return c;
}
}  // namespace detail

/// kmu_components on host arrays: the connected components of the graph over nodes 0 .. n_nodes - 1 whose edges are the records of
/// `stride` words in `edges` (words 0 and 1: the ends); with weight_at != 0 a record counts iff its word weight_at >= min_weight
/// (include/kmu.h has the rules).
inline Components components(const std::vector<uint32_t> &edges, uint32_t n_nodes, uint32_t stride = 2, uint32_t weight_at = 0,
                             uint32_t min_weight = 0, Context &ctx = Context::global()) {
    if (stride < 2 || edges.size() % stride != 0) throw std::invalid_argument("components: edges holds records of stride >= 2 words");
    const uint64_t n_edges = edges.size() / stride;
    return detail::components_call(ctx, n_nodes, [&](uint32_t *l, uint32_t *c, uint32_t *s, uint32_t *m, uint32_t *n) {
        return kmu_components(ctx.raw(), n_nodes, detail::ptr(edges), n_edges, stride, weight_at, min_weight, KMU_MEM_HOST, l, c, s, m, n);
    });
}

/// ... on the records of anchor_overlaps as they are: a record counts iff its score (by_votes: its votes) >= min_weight
inline Components components(const std::vector<kmu_overlap> &records, uint32_t n_nodes, uint32_t min_weight = 0, bool by_votes = false,
                             Context &ctx = Context::global()) {
    static_assert(sizeof(kmu_overlap) == 32, "a record is 8 words");
    return detail::components_call(ctx, n_nodes, [&](uint32_t *l, uint32_t *c, uint32_t *s, uint32_t *m, uint32_t *n) {
        return kmu_components(ctx.raw(), n_nodes, reinterpret_cast<const uint32_t *>(detail::ptr(records)), records.size(), 8, by_votes ? 5 : 4,
                              min_weight, KMU_MEM_HOST, l, c, s, m, n);
    });
}

/// kmu_components_knn on the lists of a sig_knn self-join: n_nodes rows of k entries; row i is joined to idx[i * k + j] iff
/// eq[i * k + j] >= min_eq (an empty `eq`: every entry counts, min_eq must be 0); KMU_KNN_NONE entries join nothing
inline Components components_knn(const std::vector<uint32_t> &idx, const std::vector<uint16_t> &eq, uint32_t n_nodes, uint32_t k,
                                 uint32_t min_eq = 0, Context &ctx = Context::global()) {
    if (idx.size() != size_t(n_nodes) * k) throw std::invalid_argument("components_knn: idx holds n_nodes x k entries");
    if (!eq.empty() && eq.size() != idx.size()) throw std::invalid_argument("components_knn: eq holds one value per entry of idx");
    return detail::components_call(ctx, n_nodes, [&](uint32_t *l, uint32_t *c, uint32_t *s, uint32_t *m, uint32_t *n) {
        return kmu_components_knn(ctx.raw(), n_nodes, detail::ptr(idx), detail::opt(eq), k, min_eq, KMU_MEM_HOST, l, c, s, m, n);
    });
}

/// the reads that belong together: cluster[i] of reads[i] (clusters numbered in the order of their first read), the number of reads
/// in every cluster, and the readnum of the reads ordered by (cluster, position in `reads`)
struct ReadClusters {
    std::vector<uint32_t> cluster, size, members;
};

/// read_overlaps, then the connected components of the graph whose nodes are the reads and whose edges are the overlap records
/// with score >= min_score (by_votes: the records with votes >= min_score; the vote itself then drops nothing).  A read that
/// overlaps nothing is a cluster of one.
template <class Kmer>
ReadClusters read_clusters(const std::vector<ReadAnchors<Kmer>> &reads, const AnchorsGeneratorParameters &params, uint32_t n_keys = 1,
                           uint32_t min_common = 1, uint32_t strands = 2, uint32_t band = 1, uint32_t min_score = 2,
                           uint32_t max_occ = 0, bool by_votes = false, Context &ctx = Context::global()) {
    const auto records =
        detail::read_overlap_records(reads, params, n_keys, min_common, strands, band, by_votes ? 0u : min_score, max_occ, ctx);
    Components c = components(records, uint32_t(reads.size()), min_score, by_votes, ctx);
    ReadClusters out{std::move(c.cluster), std::move(c.size), std::move(c.members)};
    for (uint32_t &r : out.members) r = reads[r].readnum;
    return out;
}

// =====================================================================================================================
// window minimizers (kmu_read_minimizers; the reference has no such unit)
// =====================================================================================================================

/// fhash of every k-mer of a batch as kmu_kmer_hashes lays them out: entry offsets[i] + p is position p of sequence i
/// (uint64, zero-extended for the u32 types); the last k - 1 entries of a sequence are 0
template <class Kmer>
std::vector<uint64_t> kmer_hashes(const detail::Batch &b, size_t k, FHash fhash, Context &ctx = Context::global()) {
    if (b.on_device()) throw std::invalid_argument("kmer_hashes returns host arrays: it needs the sequences in host memory");
    const kmu_hash_params hp = detail::hash_params<Kmer>(k, int(fhash), b.input_kind);
    std::vector<uint64_t> out(std::max<uint64_t>(b.offsets.back(), 1), 0);   // (a batch without bases gets one entry: kept as it was)
    ctx.check(kmu_kmer_hashes(ctx.raw(), &hp, b.bytes.data(), b.offsets.data(), b.packed_ptr(), b.n(), out.data()));
    return out;
}

/// kmu_minimizer_layout: win_offsets[n + 1], the windows of w k-mers of every sequence -- an upper bound of its minimizers
inline std::vector<uint64_t> minimizer_layout(const detail::Batch &b, size_t k, uint32_t w) {
    std::vector<uint64_t> win(b.offsets.size());
    const int rc = kmu_minimizer_layout(b.offsets.data(), b.n(), uint32_t(k), w, win.data());
    if (rc != KMU_OK) throw KmuError(rc, "kmu_minimizer_layout: kmer_size > 0 and 1 <= w <= KMU_MINIMIZER_MAX_W");
    return win;
}

/// The (w, k) window minimizers of a batch: entries offsets[i] .. offsets[i + 1] are those of sequence i, ascending in position;
/// hashes[e] is the kmer_hashes value of position pos[e] of sequence read[e], strand[e] = 1 iff that k-mer's reverse complement
/// is the smaller one under a canonical fhash (empty under the ntHash orders, which expose no strand).
struct Minimizers {
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> pos, read;
    std::vector<uint8_t> strand;
    std::vector<uint64_t> offsets;
    size_t size() const { return hashes.size(); }
};

/// kmu_read_minimizers in one call: the window count of kmu_minimizer_layout is the capacity, so nothing is counted first.
/// Per window of w consecutive k-mers the position of smallest hash, ties to the smallest position, each chosen position once
/// (include/kmu.h has the rules).  FHash::canon_invhash is the recommended order.
template <class Kmer>
Minimizers read_minimizers(const detail::Batch &batch, size_t k, uint32_t w, FHash fhash = FHash::canon_invhash,
                           Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("read_minimizers", batch);
    const bool with_strand = fhash != FHash::canon_nthash && fhash != FHash::canon_nthash_8b;
    const uint64_t cap = minimizer_layout(b, k, w).back();
    const kmu_hash_params hp = detail::hash_params<Kmer>(k, int(fhash), KMU_INPUT_ASCII);
    Minimizers m;
    m.hashes.assign(size_t(cap), 0);
    m.pos.assign(size_t(cap), 0);
    m.read.assign(size_t(cap), 0);
    if (with_strand) m.strand.assign(size_t(cap), 0);
    m.offsets.assign(b.offsets.size(), 0);
    uint64_t total = 0;
    ctx.check(kmu_read_minimizers(ctx.raw(), &hp, b.bytes.data(), b.offsets.data(), b.n(), w, detail::ptr(m.hashes), detail::ptr(m.pos), detail::ptr(m.read),
                                  with_strand ? detail::ptr(m.strand) : nullptr, cap, m.offsets.data(), &total));
    m.hashes.resize(size_t(total));
    m.pos.resize(size_t(total));
    m.read.resize(size_t(total));
    if (with_strand) m.strand.resize(size_t(total));
    return m;
}
template <class Kmer>
Minimizers read_minimizers(const std::vector<const Sequence *> &seqs, size_t k, uint32_t w, FHash fhash = FHash::canon_invhash,
                           Context &ctx = Context::global()) {
    return read_minimizers<Kmer>(detail::gather(seqs), k, w, fhash, ctx);
}

// =====================================================================================================================
// syncmers (kmu_read_syncmers; the reference has no such unit)
// =====================================================================================================================

/// The k-mer type the s-mers of a syncmer are hashed as: the reference's choice for s bases (_abi.kmer_type_for_k)
inline int syncmer_s_type(size_t s) { return s <= 14 ? KMU_KMER32BIT : s == 16 ? KMU_KMER16B32BIT : KMU_KMER64BIT; }

/// kmu_read_syncmers in one call: the number of k-mers (kmu_minimizer_layout with w = 1) is the capacity, so nothing is counted
/// first.  The k-mers whose smallest s-mer value sits at offset t or k - s - t: t = 0 gives closed syncmers, 2 t == k - s open
/// syncmers at the middle offset (include/kmu.h has the rules).  The s-mers are ordered by `fhash` too.  Returns the record of
/// read_minimizers: seed_pairs, chain_hits and what follows take it as it is.
template <class Kmer>
Minimizers read_syncmers(const detail::Batch &batch, size_t k, size_t s, uint32_t t = 0, FHash fhash = FHash::canon_invhash,
                         Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("read_syncmers", batch);
    const bool with_strand = fhash != FHash::canon_nthash && fhash != FHash::canon_nthash_8b;
    const uint64_t cap = minimizer_layout(b, k, 1).back();
    const kmu_hash_params hp = detail::hash_params<Kmer>(k, int(fhash), KMU_INPUT_ASCII);
    const kmu_syncmer_params sp{syncmer_s_type(s), int32_t(s), int32_t(fhash), t};
    Minimizers m;
    m.hashes.assign(size_t(cap), 0);
    m.pos.assign(size_t(cap), 0);
    m.read.assign(size_t(cap), 0);
    if (with_strand) m.strand.assign(size_t(cap), 0);
    m.offsets.assign(b.offsets.size(), 0);
    uint64_t total = 0;
    ctx.check(kmu_read_syncmers(ctx.raw(), &hp, &sp, b.bytes.data(), b.offsets.data(), b.n(), detail::ptr(m.hashes), detail::ptr(m.pos),
                                detail::ptr(m.read), with_strand ? detail::ptr(m.strand) : nullptr, cap, m.offsets.data(), &total));
    m.hashes.resize(size_t(total));
    m.pos.resize(size_t(total));
    m.read.resize(size_t(total));
    if (with_strand) m.strand.resize(size_t(total));
    return m;
}
template <class Kmer>
Minimizers read_syncmers(const std::vector<const Sequence *> &seqs, size_t k, size_t s, uint32_t t = 0, FHash fhash = FHash::canon_invhash,
                         Context &ctx = Context::global()) {
    return read_syncmers<Kmer>(detail::gather(seqs), k, s, t, fhash, ctx);
}

// =====================================================================================================================
// seed chaining (kmu_seed_chains; the reference has no such unit)
// =====================================================================================================================

namespace detail {
/// the one marshalling of both chaining entries (kmu_seed_chains, kmu_seed_chains_all): the count call, then the write call
template <class Entry>
std::vector<kmu_chain> seed_chains_with(Entry entry, const char *who, const std::vector<uint32_t> &pairs, const Minimizers &q,
                                        const Minimizers &db, const kmu_chain_params &p, Context &ctx) {
    if (q.offsets.empty() || db.offsets.empty()) throw std::invalid_argument(std::string(who) + ": offsets hold n_reads + 1 entries");
    if (q.read.size() != q.pos.size() || db.read.size() != db.pos.size() || (!q.strand.empty() && q.strand.size() != q.pos.size()) ||
        (!db.strand.empty() && db.strand.size() != db.pos.size()))
        throw std::invalid_argument(std::string(who) + ": pos, read and strand hold one value per minimizer");
    const uint64_t n_pairs = pairs.size() / 2;
    std::vector<kmu_chain> out;
    two_calls(
        ctx, false, [&](uint64_t total) { out.resize(size_t(total)); },
        [&](bool, uint64_t cap, uint64_t *total) {
            return entry(ctx.raw(), n_pairs ? pairs.data() : &spare_element<uint32_t>, n_pairs, ptr(q.pos), ptr(q.read), opt(q.strand),
                         uint32_t(q.pos.size()), uint32_t(q.offsets.size() - 1), ptr(db.pos), ptr(db.read), opt(db.strand),
                         uint32_t(db.pos.size()), uint32_t(db.offsets.size() - 1), &p, KMU_MEM_HOST, opt(out), cap, total);
        });
    return out;
}
} // namespace detail

/// kmu_seed_chains on host arrays: one chain per read pair behind `pairs` (2 per pair: an entry of q, an entry of db, in any order),
/// one kmu_chain each, ordered by (read_a, read_b) (include/kmu.h has the rules).  The count call, then the write call.
inline std::vector<kmu_chain> seed_chains(const std::vector<uint32_t> &pairs, const Minimizers &q, const Minimizers &db,
                                          const kmu_chain_params &p, Context &ctx = Context::global()) {
    return detail::seed_chains_with(kmu_seed_chains, "seed_chains", pairs, q, db, p, ctx);
}

/// kmu_seed_chains_all on host arrays: EVERY chain of every (read pair, strand) behind the same pairs, ordered by (read_a, read_b,
/// strand, end anchor) (include/kmu.h has the rules).  Arguments and the two calls are those of seed_chains.
inline std::vector<kmu_chain> seed_chains_all(const std::vector<uint32_t> &pairs, const Minimizers &q, const Minimizers &db,
                                              const kmu_chain_params &p, Context &ctx = Context::global()) {
    return detail::seed_chains_with(kmu_seed_chains_all, "seed_chains_all", pairs, q, db, p, ctx);
}

/// kmu_chain_rank on host arrays: rank, parent, sub_score and n_sub of every chain inside its query read, aligned with `chains`
/// (the chains of one read_a together, read_a ascending: as both chaining entries write them; include/kmu.h has the rules).
inline std::vector<kmu_chain_rank_rec> chain_rank(const std::vector<kmu_chain> &chains, uint32_t n_reads_q, uint32_t mask_permille = 500,
                                                  Context &ctx = Context::global()) {
    std::vector<kmu_chain_rank_rec> out(chains.size());
    if (chains.empty()) return out;
    kmu_rank_params p{};
    p.mask_permille = mask_permille;
    ctx.check(kmu_chain_rank(ctx.raw(), chains.data(), chains.size(), n_reads_q, &p, KMU_MEM_HOST, out.data()));
    return out;
}

/// The mapping quality of chain `at` (minimizer.chain_mapq), host code: for a primary min(60, floor(40 * (1 - sub_score / score) *
/// min(1, n_seeds / 10) * ln(score))) in doubles, the formula of the minimap2 paper; 0 for a secondary and for a score of 0.
inline uint32_t chain_mapq(const kmu_chain &c, const kmu_chain_rank_rec &r, size_t at) {
    if (r.parent != at || c.score == 0) return 0;
    const double q = 40.0 * (1.0 - double(r.sub_score) / double(c.score)) * std::min(1.0, double(c.n_seeds) / 10.0) * std::log(double(c.score));
    return uint32_t(std::min(60.0, std::floor(q)));
}

/// The index join behind chain_hits: the pairs (entry of q, entry of db; 2 per pair) of minimizers that carry the same hash, through
/// an AnchorIndex of rows of one hash.  db == nullptr: the self-join of q, a minimizer never pairs with one of its own read.
/// max_occ > 0: a hash that more than max_occ minimizers of db carry seeds nothing.
inline std::vector<uint32_t> seed_pairs(const Minimizers &q, const Minimizers *db = nullptr, uint32_t max_occ = 0,
                                        Context &ctx = Context::global()) {
    const Minimizers &d = db ? *db : q;
    const std::vector<uint32_t> no_group;
    std::vector<uint32_t> pairs, dist;
    if (q.size() == 0 || d.size() == 0) return pairs;
    AnchorIndex(d.hashes, uint32_t(d.size()), 1, 1, db ? no_group : d.read, ctx)
        .match(q.hashes, uint32_t(q.size()), db ? no_group : q.read, 1, max_occ, pairs, dist);
    return pairs;
}

/// From minimizers to one chain per read pair: seed_pairs, then seed_chains.  `span` is the k of the minimizers.  The self-join
/// (db == nullptr) reports each read pair once, read_a < read_b.
inline std::vector<kmu_chain> chain_hits(const Minimizers &q, const Minimizers *db, uint32_t span, uint32_t max_occ = 0,
                                         uint32_t max_gap = 5000, uint32_t band = 500, uint32_t min_seeds = 3, uint32_t min_score = 0,
                                         Context &ctx = Context::global()) {
    kmu_chain_params p{};
    p.span = span;
    p.max_gap = max_gap;
    p.band = band;
    p.min_seeds = min_seeds;
    p.min_score = min_score;
    p.flags = db ? 0u : KMU_CHAIN_UPPER;
    return seed_chains(seed_pairs(q, db, max_occ, ctx), q, db ? *db : q, p, ctx);
}
/// The same with the switch of the Python route (minimizer.chain_hits(..., all=...)): all == true reports every chain of every read
/// pair (seed_chains_all), which is what mapping reads onto contigs needs.
inline std::vector<kmu_chain> chain_hits(const Minimizers &q, const Minimizers *db, uint32_t span, uint32_t max_occ, uint32_t max_gap,
                                         uint32_t band, uint32_t min_seeds, uint32_t min_score, Context &ctx, bool all) {
    if (!all) return chain_hits(q, db, span, max_occ, max_gap, band, min_seeds, min_score, ctx);
    kmu_chain_params p{};
    p.span = span;
    p.max_gap = max_gap;
    p.band = band;
    p.min_seeds = min_seeds;
    p.min_score = min_score;
    p.flags = db ? 0u : KMU_CHAIN_UPPER;
    return seed_chains_all(seed_pairs(q, db, max_occ, ctx), q, db ? *db : q, p, ctx);
}

/// From the reads of a batch to the chains between them: read_minimizers, then the self-join of chain_hits.
template <class Kmer>
std::vector<kmu_chain> read_chains(const detail::Batch &batch, size_t k, uint32_t w, FHash fhash = FHash::canon_invhash,
                                   uint32_t max_occ = 0, uint32_t max_gap = 5000, uint32_t band = 500, uint32_t min_seeds = 3,
                                   uint32_t min_score = 0, Context &ctx = Context::global()) {
    const Minimizers m = read_minimizers<Kmer>(batch, k, w, fhash, ctx);
    return chain_hits(m, nullptr, uint32_t(k), max_occ, max_gap, band, min_seeds, min_score, ctx);
}
/// The same with the switch of the Python route (minimizer.read_chains(..., all=...))
template <class Kmer>
std::vector<kmu_chain> read_chains(const detail::Batch &batch, size_t k, uint32_t w, FHash fhash, uint32_t max_occ, uint32_t max_gap,
                                   uint32_t band, uint32_t min_seeds, uint32_t min_score, Context &ctx, bool all) {
    const Minimizers m = read_minimizers<Kmer>(batch, k, w, fhash, ctx);
    return chain_hits(m, nullptr, uint32_t(k), max_occ, max_gap, band, min_seeds, min_score, ctx, all);
}

// =====================================================================================================================
// chain alignment (kmu_chain_align; the reference has no such unit)
// =====================================================================================================================

/// kmu_chain_align on host arrays: for every chain record the banded global alignment of the two segments it names -- edit distance,
/// matching columns, the diagonals of its band and the flags KMU_ALN_DONE / KMU_ALN_EXACT (include/kmu.h has the rules).  q, db:
/// the batches the chains' reads are numbered in (db == nullptr: the self-join on one batch); packed batches are unpacked first.
inline std::vector<kmu_chain_aln> chain_align(const std::vector<kmu_chain> &chains, const detail::Batch &q, const detail::Batch *db = nullptr,
                                              uint32_t band = 64, Context &ctx = Context::global()) {
    const detail::Sides both = detail::host_sides("chain_align", q, db);
    const detail::Batch &bq = both.q, &bdb = both.db();
    std::vector<kmu_chain_aln> out(chains.size());
    if (chains.empty()) return out;
    kmu_align_params p{};
    p.band = band;
    ctx.check(kmu_chain_align(ctx.raw(), chains.data(), chains.size(), bq.bytes.data(), bq.offsets.data(), bq.n(), bdb.bytes.data(),
                              bdb.offsets.data(), bdb.n(), &p, KMU_MEM_HOST, out.data()));
    return out;
}
/// The same under the name of the Python route (minimizer.align_chains)
inline std::vector<kmu_chain_aln> align_chains(const std::vector<kmu_chain> &chains, const detail::Batch &q, const detail::Batch *db = nullptr,
                                               uint32_t band = 64, Context &ctx = Context::global()) {
    return chain_align(chains, q, db, band, ctx);
}

/// From the reads of a batch to the chains between them and their alignments: read_chains (band_chain is its band), then
/// chain_align with `band`.
template <class Kmer>
std::pair<std::vector<kmu_chain>, std::vector<kmu_chain_aln>> read_alignments(const detail::Batch &batch, size_t k, uint32_t w,
                                                                              FHash fhash = FHash::canon_invhash, uint32_t max_occ = 0,
                                                                              uint32_t max_gap = 5000, uint32_t band_chain = 500,
                                                                              uint32_t min_seeds = 3, uint32_t min_score = 0,
                                                                              uint32_t band = 64, Context &ctx = Context::global()) {
    std::vector<kmu_chain> chains = read_chains<Kmer>(batch, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, ctx);
    std::vector<kmu_chain_aln> aln = chain_align(chains, batch, nullptr, band, ctx);
    return {std::move(chains), std::move(aln)};
}

/// One PAF line (no newline) of a chain and its alignment: the 12 standard columns -- query name, length, start, end, strand, target
/// name, length, start, end, matches, matches + edit, mapq 255 -- then NM:i:edit, s1:i:score and cm:i:n_seeds.  A record without
/// KMU_ALN_DONE writes 0 matches, a block of max(m, n) and no NM tag.  Host code.
inline std::string paf_line(const kmu_chain &c, const kmu_chain_aln &a, const std::string &name_q, uint64_t len_q,
                            const std::string &name_db, uint64_t len_db) {
    const bool done = (a.flags & KMU_ALN_DONE) != 0;
    const uint64_t block = done ? uint64_t(a.matches) + a.edit : std::max<uint64_t>(c.a_end - c.a_start, c.b_end - c.b_start);
    std::string s = name_q + "\t" + std::to_string(len_q) + "\t" + std::to_string(c.a_start) + "\t" + std::to_string(c.a_end) + "\t" +
                    (c.strand ? "-" : "+") + "\t" + name_db + "\t" + std::to_string(len_db) + "\t" + std::to_string(c.b_start) + "\t" +
                    std::to_string(c.b_end) + "\t" + std::to_string(done ? a.matches : 0u) + "\t" + std::to_string(block) + "\t255";
    if (done) s += "\tNM:i:" + std::to_string(a.edit);
    return s + "\ts1:i:" + std::to_string(c.score) + "\tcm:i:" + std::to_string(c.n_seeds);
}

/// paf_line with the record of chain_rank for chain `at` of its array: column 12 is chain_mapq, and tp:A:P (primary) or tp:A:S
/// (secondary) and s2:i:sub_score follow cm:i:.
inline std::string paf_line(const kmu_chain &c, const kmu_chain_aln &a, const kmu_chain_rank_rec &r, size_t at, const std::string &name_q,
                            uint64_t len_q, const std::string &name_db, uint64_t len_db) {
    std::string s = paf_line(c, a, name_q, len_q, name_db, len_db);
    size_t tab = 0; // where column 12 begins: behind the eleventh tab (names hold none)
    for (int col = 0; col < 11; col++) tab = s.find('\t', tab) + 1;
    const size_t end = s.find('\t', tab);
    s.replace(tab, end - tab, std::to_string(chain_mapq(c, r, at)));
    return s + "\ttp:A:" + (r.parent == at ? "P" : "S") + "\ts2:i:" + std::to_string(r.sub_score);
}

// =====================================================================================================================
// chain alignment paths (kmu_chain_cigar; the reference has no such unit)
// =====================================================================================================================

/// What chain_cigar returns: the records of chain_align with KMU_ALN_PATH where a chain's runs were written, and the runs
/// (len << 4 | KMU_CIGAR_*) of chain c in ops[op_offsets[c] .. op_offsets[c + 1]), in path order along A.
struct ChainCigars {
    std::vector<kmu_chain_aln> aln;
    std::vector<uint32_t> ops;
    std::vector<uint64_t> op_offsets;
};

/// kmu_chain_cigar on host arrays: chain_align and, for every chain, the path of its alignment as CIGAR runs (include/kmu.h has
/// the rules).  Arguments as chain_align; max_trace_bytes: the workspace the direction bits of one batch of chains may take
/// (0: KMU_CIGAR_TRACE_DEFAULT).  Two library calls: one that counts, one with exactly that capacity.
inline ChainCigars chain_cigar(const std::vector<kmu_chain> &chains, const detail::Batch &q, const detail::Batch *db = nullptr,
                               uint32_t band = 64, uint64_t max_trace_bytes = 0, Context &ctx = Context::global()) {
    const detail::Sides both = detail::host_sides("chain_cigar", q, db);
    const detail::Batch &bq = both.q, &bdb = both.db();
    ChainCigars out;
    out.aln.resize(chains.size());
    out.op_offsets.assign(chains.size() + 1, 0);
    if (chains.empty()) return out;
    kmu_cigar_params p{};
    p.band = band;
    p.max_trace_bytes = max_trace_bytes;
    detail::two_calls(
        ctx, false, [&](uint64_t total) { out.ops.resize(total); },
        [&](bool, uint64_t cap, uint64_t *total) {
            return kmu_chain_cigar(ctx.raw(), chains.data(), chains.size(), bq.bytes.data(), bq.offsets.data(), bq.n(), bdb.bytes.data(),
                                   bdb.offsets.data(), bdb.n(), &p, KMU_MEM_HOST, out.aln.data(), out.op_offsets.data(), detail::opt(out.ops), cap, total);
        });
    return out;
}
/// The same under the name of the Python route (minimizer.cigar_chains)
inline ChainCigars cigar_chains(const std::vector<kmu_chain> &chains, const detail::Batch &q, const detail::Batch *db = nullptr,
                                uint32_t band = 64, uint64_t max_trace_bytes = 0, Context &ctx = Context::global()) {
    return chain_cigar(chains, q, db, band, max_trace_bytes, ctx);
}

/// The runs of chain c as a CIGAR string ("" for a chain without runs).  extended == false merges = and X into M; reversed writes
/// the runs in reverse order -- for a chain on strand 1, along the forward strand of the target, as PAF's cg tag wants them.  Host code.
inline std::string cigar_string(const ChainCigars &r, size_t c, bool extended = true, bool reversed = false) {
    std::vector<std::pair<uint64_t, char>> runs;
    for (uint64_t x = r.op_offsets[c]; x < r.op_offsets[c + 1]; x++) {
        const uint32_t op = r.ops[x] & 15u;
        char letter = op == KMU_CIGAR_I ? 'I' : op == KMU_CIGAR_D ? 'D' : op == KMU_CIGAR_EQ ? '=' : 'X';
        if (!extended && (letter == '=' || letter == 'X')) letter = 'M';
        runs.emplace_back(r.ops[x] >> 4, letter);
    }
    if (reversed) std::reverse(runs.begin(), runs.end());
    std::string s;
    for (size_t x = 0; x < runs.size(); x++) {
        uint64_t n = runs[x].first;
        while (x + 1 < runs.size() && runs[x + 1].second == runs[x].second) n += runs[++x].first;
        s += std::to_string(n) + runs[x].second;
    }
    return s;
}

/// paf_line with the cg:Z: tag: the runs of chain c of `cigars`, along the target's forward strand, where its record has
/// KMU_ALN_PATH; the line of the overload above otherwise.
inline std::string paf_line(const kmu_chain &c, const ChainCigars &cigars, size_t at, const std::string &name_q, uint64_t len_q,
                            const std::string &name_db, uint64_t len_db) {
    std::string s = paf_line(c, cigars.aln[at], name_q, len_q, name_db, len_db);
    if (cigars.aln[at].flags & KMU_ALN_PATH) s += "\tcg:Z:" + cigar_string(cigars, at, true, c.strand != 0);
    return s;
}

// =====================================================================================================================
// read pileup (kmu_chain_pileup, kmu_pile_call; the reference has no such unit)
// =====================================================================================================================

/// What chain_pileup returns: one row of KMU_PILE_COLS counts per base of a batch (include/kmu.h has the columns).  In the
/// self-join both sides vote into ONE table, `q`, and `shared` is set; otherwise `q` belongs to the q batch and `db` to the db batch
/// (a side that was not asked for is empty).
struct ChainPileups {
    std::vector<uint32_t> q, db;
    bool shared = false;
    const std::vector<uint32_t> &of_db() const { return shared ? q : db; }
    /// A + C + G + T + DEL of a row of `table`
    static uint64_t depth(const std::vector<uint32_t> &table, uint64_t row) {
        uint64_t d = 0;
        for (uint32_t k = 0; k <= KMU_PILE_DEL; k++) d += table[row * KMU_PILE_COLS + k];
        return d;
    }
};

namespace detail {
/// the records and run offsets of `cigars` are those of `chains` (lib.py's _runs_of_chains)
inline void cigars_of_chains(const char *who, const std::vector<kmu_chain> &chains, const ChainCigars &cigars) {
    if (cigars.aln.size() != chains.size() || cigars.op_offsets.size() != chains.size() + 1)
        throw std::invalid_argument(std::string(who) + ": the records and run offsets are not those of the chains");
}
/// The vote tables of the two sides (lib.py's _side_tables), grown to size_q and size_db entries where they are voted into: the
/// self-join (`two` false) has ONE table, q, also when only the B side votes, and `shared` says that both sides vote into it.
template <class Tables> void side_tables(Tables &out, bool two, uint32_t sides, size_t size_q, size_t size_db) {
    out.shared = !two && (sides & KMU_PILE_Q) && (sides & KMU_PILE_DB);
    const bool db_in_q = !two && !(sides & KMU_PILE_Q);
    if ((sides & KMU_PILE_Q) || db_in_q) out.q.resize(size_q, 0u);
    if ((sides & KMU_PILE_DB) && two) out.db.resize(size_db, 0u);
}
}  // namespace detail

/// kmu_chain_pileup on host arrays: the votes of every chain's runs onto the bases of both reads.  chains and cigars: the chains
/// given to chain_cigar and what it returned; q, db as there (db == nullptr: the self-join, one shared table); sides: KMU_PILE_Q,
/// KMU_PILE_DB or both.  into: tables of an earlier call on the same batches to add to (moved from).
inline ChainPileups chain_pileup(const std::vector<kmu_chain> &chains, const ChainCigars &cigars, const detail::Batch &q,
                                 const detail::Batch *db = nullptr, uint32_t sides = KMU_PILE_Q | KMU_PILE_DB, ChainPileups into = {},
                                 Context &ctx = Context::global()) {
    const detail::Sides both = detail::host_sides("chain_pileup", q, db);
    const detail::Batch &bq = both.q, &bdb = both.db();
    detail::cigars_of_chains("chain_pileup", chains, cigars);
    ChainPileups out = std::move(into);
    detail::side_tables(out, both.two, sides, size_t(bq.offsets.back()) * KMU_PILE_COLS, size_t(bdb.offsets.back()) * KMU_PILE_COLS);
    if (chains.empty()) return out;
    kmu_pileup_params p{};
    p.flags = sides;
    uint32_t *table_db = db ? out.db.data() : out.q.data();
    ctx.check(kmu_chain_pileup(ctx.raw(), chains.data(), chains.size(), cigars.aln.data(), cigars.op_offsets.data(), cigars.ops.data(),
                               cigars.ops.size(), bq.bytes.data(), bq.offsets.data(), bq.n(), bdb.bytes.data(), bdb.offsets.data(), bdb.n(), &p,
                               KMU_MEM_HOST, (sides & KMU_PILE_Q) ? out.q.data() : nullptr, (sides & KMU_PILE_DB) ? table_db : nullptr));
    return out;
}
/// The same under the name of the Python route (minimizer.pileup_chains)
inline ChainPileups pileup_chains(const std::vector<kmu_chain> &chains, const ChainCigars &cigars, const detail::Batch &q,
                                  const detail::Batch *db = nullptr, uint32_t sides = KMU_PILE_Q | KMU_PILE_DB, ChainPileups into = {},
                                  Context &ctx = Context::global()) {
    return chain_pileup(chains, cigars, q, db, sides, std::move(into), ctx);
}

/// What pile_call returns: the call byte of every base (code | KMU_CALL_INS | KMU_CALL_DIFF, KMU_CALL_NONE below min_depth) and the
/// summary of every read.
struct PileCalls {
    std::vector<uint8_t> call;
    std::vector<kmu_read_pile> reads;
};

/// kmu_pile_call on host arrays: `table` is a table of chain_pileup for `batch`.
inline PileCalls pile_call(const std::vector<uint32_t> &table, const detail::Batch &batch, uint32_t min_depth = 3, Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("pile_call", batch);
    if (table.size() != size_t(b.offsets.back()) * KMU_PILE_COLS) throw std::invalid_argument("pile_call: the table is not one of this batch");
    PileCalls out;
    out.call.resize(b.offsets.back());
    out.reads.resize(b.n());
    if (!b.n()) return out;
    kmu_pile_call_params p{};
    p.min_depth = min_depth;
    ctx.check(kmu_pile_call(ctx.raw(), detail::ptr(table), detail::ptr(b.bytes), b.offsets.data(), b.n(), &p, KMU_MEM_HOST, detail::ptr(out.call),
                            out.reads.data()));
    return out;
}

// =====================================================================================================================
// read correction (kmu_pile_ins_plan, kmu_chain_pile_ins, kmu_pile_consensus; the reference has no such unit)
// =====================================================================================================================

/// What pile_ins_plan returns: the number of insertion slots of every base of a batch, and their sum.  Slot s of row g has the index
/// S(g) + s, S being the exclusive prefix sum of ins_len.
struct InsPlan {
    std::vector<uint8_t> ins_len;
    uint64_t n_slots = 0;
};

/// kmu_pile_ins_plan on host arrays: `table` is a table of chain_pileup and `call` the call bytes pile_call made from it.
inline InsPlan pile_ins_plan(const std::vector<uint32_t> &table, const std::vector<uint8_t> &call, uint32_t max_ins = 16,
                             Context &ctx = Context::global()) {
    if (table.size() != call.size() * KMU_PILE_COLS) throw std::invalid_argument("pile_ins_plan: the table and the calls are not of one batch");
    InsPlan out;
    out.ins_len.resize(call.size());
    kmu_ins_plan_params p{};
    p.max_ins = max_ins;
    ctx.check(kmu_pile_ins_plan(ctx.raw(), detail::ptr(table), detail::ptr(call), call.size(), &p, KMU_MEM_HOST, detail::ptr(out.ins_len), &out.n_slots));
    return out;
}

/// What chain_pile_ins returns: KMU_INS_COLS counts (A C G T) per insertion slot of a batch.  As in ChainPileups, the self-join votes
/// into ONE table, `q`, and `shared` is set.
struct ChainInsertions {
    std::vector<uint32_t> q, db;
    bool shared = false;
    const std::vector<uint32_t> &of_db() const { return shared ? q : db; }
};

/// kmu_chain_pile_ins on host arrays: the letters of every chain's gap runs, voted into the slots of both reads.  chains, cigars, q,
/// db, sides as chain_pileup takes them; plan_q / plan_db: pile_ins_plan of each batch (plan_db == nullptr in the self-join).  into:
/// tables of an earlier call with the same plans to add to (moved from).
inline ChainInsertions chain_pile_ins(const std::vector<kmu_chain> &chains, const ChainCigars &cigars, const detail::Batch &q, const InsPlan &plan_q,
                                      const detail::Batch *db = nullptr, const InsPlan *plan_db = nullptr, uint32_t sides = KMU_PILE_Q | KMU_PILE_DB,
                                      ChainInsertions into = {}, Context &ctx = Context::global()) {
    const detail::Sides both = detail::host_sides("chain_pile_ins", q, db);
    const detail::Batch &bq = both.q, &bdb = both.db();
    detail::cigars_of_chains("chain_pile_ins", chains, cigars);
    if (bool(db) != bool(plan_db)) throw std::invalid_argument("chain_pile_ins: a db batch and its plan come together");
    const InsPlan &pdb = db ? *plan_db : plan_q;
    if (plan_q.ins_len.size() != bq.offsets.back() || pdb.ins_len.size() != bdb.offsets.back())
        throw std::invalid_argument("chain_pile_ins: a plan is not one of its batch");
    ChainInsertions out = std::move(into);
    detail::side_tables(out, both.two, sides, size_t(plan_q.n_slots) * KMU_INS_COLS, size_t(pdb.n_slots) * KMU_INS_COLS);
    if (chains.empty()) return out;
    kmu_pileup_params p{};
    p.flags = sides;
    uint32_t none_db = 0; // the db table's own spare: the library takes two equal table addresses for the self-join's one table
    uint32_t *table_q = detail::ptr(out.q);
    uint32_t *table_db = !db ? table_q : out.db.empty() ? &none_db : out.db.data();
    ctx.check(kmu_chain_pile_ins(ctx.raw(), chains.data(), chains.size(), cigars.aln.data(), cigars.op_offsets.data(), cigars.ops.data(),
                                 cigars.ops.size(), bq.bytes.data(), bq.offsets.data(), bq.n(), bdb.bytes.data(), bdb.offsets.data(), bdb.n(), &p,
                                 KMU_MEM_HOST, detail::ptr(plan_q.ins_len), plan_q.n_slots, (sides & KMU_PILE_Q) ? table_q : nullptr,
                                 detail::ptr(pdb.ins_len), pdb.n_slots, (sides & KMU_PILE_DB) ? table_db : nullptr));
    return out;
}
/// The same under the name of the Python route (minimizer.insertions_chains)
inline ChainInsertions insertions_chains(const std::vector<kmu_chain> &chains, const ChainCigars &cigars, const detail::Batch &q, const InsPlan &plan_q,
                                         const detail::Batch *db = nullptr, const InsPlan *plan_db = nullptr,
                                         uint32_t sides = KMU_PILE_Q | KMU_PILE_DB, ChainInsertions into = {}, Context &ctx = Context::global()) {
    return chain_pile_ins(chains, cigars, q, plan_q, db, plan_db, sides, std::move(into), ctx);
}

/// What pile_consensus returns: the corrected reads as a new ASCII batch -- read r is bases[offsets[r] .. offsets[r + 1]).
struct ConsensusReads {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets;
    std::string read(size_t r) const { return std::string(bases.begin() + offsets[r], bases.begin() + offsets[r + 1]); }
};

namespace detail {
/// the host batch of a consensus call, once its table, calls, plan and slots were found to be of that batch (lib.py's _consensus_inputs)
inline Batch consensus_inputs(const char *who, const std::vector<uint32_t> &table, const std::vector<uint8_t> &call, const InsPlan &plan,
                              const std::vector<uint32_t> &ins, const Batch &batch) {
    Batch b = host_batch(who, batch);
    const size_t n_bases = b.offsets.back();
    if (table.size() != n_bases * KMU_PILE_COLS || call.size() != n_bases || plan.ins_len.size() != n_bases || ins.size() != plan.n_slots * KMU_INS_COLS)
        throw std::invalid_argument(std::string(who) + ": the table, the calls, the plan or the slots are not of this batch");
    return b;
}
}  // namespace detail

/// kmu_pile_consensus on host arrays: table, call, plan and ins (a table of chain_pile_ins) belong to `batch`.  A row gives at most
/// one byte and its slots, so the output is sized by n_bases + n_slots and the library is called once.
inline ConsensusReads pile_consensus(const std::vector<uint32_t> &table, const std::vector<uint8_t> &call, const InsPlan &plan,
                                     const std::vector<uint32_t> &ins, const detail::Batch &batch, Context &ctx = Context::global()) {
    using detail::ptr;
    const detail::Batch b = detail::consensus_inputs("pile_consensus", table, call, plan, ins, batch);
    ConsensusReads out;
    out.offsets.assign(size_t(b.n()) + 1, 0);
    out.bases.resize(size_t(b.offsets.back()) + plan.n_slots + 1);   // (the capacity the library is told: one more than the bound, kept as it was)
    kmu_consensus_params p{};
    uint64_t total = 0;
    ctx.check(kmu_pile_consensus(ctx.raw(), ptr(table), ptr(call), ptr(plan.ins_len), plan.n_slots, detail::opt(ins), ptr(b.bytes), b.offsets.data(), b.n(),
                                 &p, KMU_MEM_HOST, out.offsets.data(), out.bases.data(), out.bases.size(), &total));
    out.bases.resize(total);
    return out;
}
/// The same under the name of the Python route (minimizer.consensus_reads)
inline ConsensusReads consensus_reads(const std::vector<uint32_t> &table, const std::vector<uint8_t> &call, const InsPlan &plan,
                                      const std::vector<uint32_t> &ins, const detail::Batch &batch, Context &ctx = Context::global()) {
    return pile_consensus(table, call, plan, ins, batch, ctx);
}

/// What correct_reads returns: the corrected reads and the summaries of pile_call.
struct CorrectedReads {
    ConsensusReads cons;
    std::vector<kmu_read_pile> reads;
};

/// The corrected reads of the chains of a batch's self-join: chain_cigar, chain_pileup, pile_call with `min_depth`, pile_ins_plan with
/// `max_ins`, chain_pile_ins, pile_consensus.
inline CorrectedReads correct_chains(const std::vector<kmu_chain> &chains, const detail::Batch &batch, uint32_t band = 64, uint32_t min_depth = 3,
                                     uint32_t max_ins = 16, Context &ctx = Context::global()) {
    const ChainCigars cigars = chain_cigar(chains, batch, nullptr, band, 0, ctx);
    const ChainPileups pile = chain_pileup(chains, cigars, batch, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx);
    PileCalls calls = pile_call(pile.q, batch, min_depth, ctx);
    const InsPlan plan = pile_ins_plan(pile.q, calls.call, max_ins, ctx);
    const ChainInsertions ins = chain_pile_ins(chains, cigars, batch, plan, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx);
    return {pile_consensus(pile.q, calls.call, plan, ins.q, batch, ctx), std::move(calls.reads)};
}

/// From the reads of a batch to their corrected versions (minimizer.correct_reads): read_chains (band_chain is its band), then
/// correct_chains.
template <class Kmer>
CorrectedReads correct_reads(const detail::Batch &batch, size_t k, uint32_t w, FHash fhash = FHash::canon_invhash, uint32_t max_occ = 0,
                             uint32_t max_gap = 5000, uint32_t band_chain = 500, uint32_t min_seeds = 3, uint32_t min_score = 0, uint32_t band = 64,
                             uint32_t min_depth = 3, uint32_t max_ins = 16, Context &ctx = Context::global()) {
    return correct_chains(read_chains<Kmer>(batch, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, ctx), batch, band, min_depth,
                          max_ins, ctx);
}

// =====================================================================================================================
// read trimming (kmu_pile_segments, kmu_extract_ranges, kmu_pile_consensus_pos; the reference has no such unit)
// =====================================================================================================================

/// What pile_segments returns: the kept segments in (read, start) order, the first listed segment of every read, and the summary
/// of every read with its class KMU_TRIM_*.
struct PileSegments {
    std::vector<kmu_pile_seg> segs;
    std::vector<uint64_t> seg_offsets;
    std::vector<kmu_read_trim> reads;
};

/// kmu_pile_segments on host arrays: `table` is a table of chain_pileup for the batch with these offsets.  A segment is a maximal run
/// of rows with depth >= min_depth in which consecutive rows are linked by a spanning depth >= min_span (0: depth only); segments of
/// at least min_len rows are kept.  longest: list only the longest kept segment of every read.  Kept segments are disjoint and at
/// least min_len long, so the output is sized by n_bases / min_len and the library is called once.
inline PileSegments pile_segments(const std::vector<uint32_t> &table, const std::vector<uint64_t> &offsets, uint32_t min_depth = 3, uint32_t min_span = 3,
                                  uint32_t min_len = 1, bool longest = false, Context &ctx = Context::global()) {
    if (offsets.empty() || table.size() != size_t(offsets.back()) * KMU_PILE_COLS) throw std::invalid_argument("pile_segments: the table is not one of this batch");
    PileSegments out;
    const uint32_t n_reads = uint32_t(offsets.size() - 1);
    const size_t n_bases = offsets.back(), by_len = n_bases / (min_len ? min_len : 1), cap = longest && n_reads < by_len ? n_reads : by_len;
    out.seg_offsets.assign(size_t(n_reads) + 1, 0);
    out.segs.resize(cap);
    out.reads.resize(n_reads);
    kmu_pile_seg_params p{};
    p.min_depth = min_depth;
    p.min_span = min_span;
    p.min_len = min_len;
    p.flags = longest ? KMU_SEG_LONGEST : 0u;
    uint64_t total = 0;
    ctx.check(kmu_pile_segments(ctx.raw(), detail::ptr(table), offsets.data(), n_reads, &p, KMU_MEM_HOST, out.seg_offsets.data(), detail::ptr(out.segs), cap,
                                &total, detail::opt(out.reads)));
    out.segs.resize(total);
    return out;
}

/// kmu_extract_ranges on host arrays: a new batch whose read i is bases[begin[i] .. end[i]), verbatim.  Ranges may be empty, overlap,
/// repeat and come in any order; a range with begin > end or end > bases.size() is refused.
inline ConsensusReads extract_ranges(const std::vector<uint8_t> &bases, const std::vector<uint64_t> &begin, const std::vector<uint64_t> &end,
                                     Context &ctx = Context::global()) {
    if (begin.size() != end.size()) throw std::invalid_argument("extract_ranges: as many ends as begins");
    ConsensusReads out;
    out.offsets.assign(begin.size() + 1, 0);
    detail::two_calls(
        ctx, false, [&](uint64_t total) { out.bases.resize(total); },
        [&](bool, uint64_t cap, uint64_t *total) {
            return kmu_extract_ranges(ctx.raw(), detail::ptr(bases), bases.size(), detail::ptr(begin), detail::ptr(end), begin.size(), KMU_MEM_HOST,
                                      out.offsets.data(), detail::opt(out.bases), cap, total);
        });
    return out;
}

/// kmu_pile_consensus_pos on host arrays: for every named row of the batch, the number of consensus bytes that the rows before it
/// produce (rows[i] == n_bases: the total).  The inputs are those of pile_consensus; rows = the batch's offsets gives its offsets.
inline std::vector<uint64_t> pile_consensus_pos(const std::vector<uint32_t> &table, const std::vector<uint8_t> &call, const InsPlan &plan,
                                                const std::vector<uint32_t> &ins, const detail::Batch &batch, const std::vector<uint64_t> &rows,
                                                Context &ctx = Context::global()) {
    using detail::opt;
    using detail::ptr;
    const detail::Batch b = detail::consensus_inputs("pile_consensus_pos", table, call, plan, ins, batch);
    std::vector<uint64_t> pos(rows.size(), 0);
    kmu_consensus_params p{};
    ctx.check(kmu_pile_consensus_pos(ctx.raw(), ptr(table), ptr(call), ptr(plan.ins_len), plan.n_slots, opt(ins), ptr(b.bytes), b.offsets.data(), b.n(), &p,
                                     KMU_MEM_HOST, opt(rows), rows.size(), opt(pos)));
    return pos;
}

/// What trim_reads returns: the trimmed (and split) reads as a new ASCII batch, the segments its reads are, and the summary of every
/// input read.
struct TrimmedReads {
    ConsensusReads out;
    std::vector<kmu_pile_seg> segs;
    std::vector<kmu_read_trim> reads;
};

namespace detail {
/// (first row, end row) of every segment in its batch
inline void segment_rows(const std::vector<kmu_pile_seg> &segs, const std::vector<uint64_t> &offsets, std::vector<uint64_t> &first, std::vector<uint64_t> &last) {
    for (const kmu_pile_seg &s : segs) {
        first.push_back(offsets[s.read] + s.start);
        last.push_back(offsets[s.read] + s.end);
    }
}
} // namespace detail

/// The reads of a batch cut down to their supported segments (minimizer.trim_reads): pile_segments on `table`, extract_ranges on the
/// batch's bytes.  Every kept segment becomes a read: uncovered ends go, a chimera comes out as its parts.
inline TrimmedReads trim_reads(const std::vector<uint32_t> &table, const detail::Batch &batch, uint32_t min_depth = 3, uint32_t min_span = 3,
                               uint32_t min_len = 100, bool longest = false, Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("trim_reads", batch);
    PileSegments s = pile_segments(table, b.offsets, min_depth, min_span, min_len, longest, ctx);
    std::vector<uint64_t> first, last;
    detail::segment_rows(s.segs, b.offsets, first, last);
    return {extract_ranges(b.bytes, first, last, ctx), std::move(s.segs), std::move(s.reads)};
}

/// What correct_trim_reads returns: the corrected, trimmed and split reads, the segments (in raw read coordinates) they are, the
/// summaries of pile_call and those of pile_segments.
struct CorrectedTrimmedReads {
    ConsensusReads out;
    std::vector<kmu_pile_seg> segs;
    std::vector<kmu_read_pile> reads;
    std::vector<kmu_read_trim> trims;
};

/// correct_chains and trim_reads on one table: the consensus of every read, the segments of the same table, pile_consensus_pos of
/// every segment's first row and end row, extract_ranges on the consensus batch.
inline CorrectedTrimmedReads correct_trim_chains(const std::vector<kmu_chain> &chains, const detail::Batch &batch, uint32_t band = 64, uint32_t min_depth = 3,
                                                 uint32_t max_ins = 16, uint32_t min_span = 3, uint32_t min_len = 100, bool longest = false,
                                                 Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("correct_trim_chains", batch);
    const ChainCigars cigars = chain_cigar(chains, batch, nullptr, band, 0, ctx);
    const ChainPileups pile = chain_pileup(chains, cigars, batch, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx);
    PileCalls calls = pile_call(pile.q, batch, min_depth, ctx);
    const InsPlan plan = pile_ins_plan(pile.q, calls.call, max_ins, ctx);
    const ChainInsertions ins = chain_pile_ins(chains, cigars, batch, plan, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx);
    const ConsensusReads cons = pile_consensus(pile.q, calls.call, plan, ins.q, batch, ctx);
    PileSegments s = pile_segments(pile.q, b.offsets, min_depth, min_span, min_len, longest, ctx);
    std::vector<uint64_t> rows, last;
    detail::segment_rows(s.segs, b.offsets, rows, last);
    const size_t n = rows.size();
    rows.insert(rows.end(), last.begin(), last.end());
    const std::vector<uint64_t> pos = pile_consensus_pos(pile.q, calls.call, plan, ins.q, batch, rows, ctx);
    return {extract_ranges(cons.bases, std::vector<uint64_t>(pos.begin(), pos.begin() + n), std::vector<uint64_t>(pos.begin() + n, pos.end()), ctx),
            std::move(s.segs), std::move(calls.reads), std::move(s.reads)};
}

/// From the reads of a batch to their corrected and trimmed versions (minimizer.correct_trim_reads): read_chains, then
/// correct_trim_chains.
template <class Kmer>
CorrectedTrimmedReads correct_trim_reads(const detail::Batch &batch, size_t k, uint32_t w, FHash fhash = FHash::canon_invhash, uint32_t max_occ = 0,
                                         uint32_t max_gap = 5000, uint32_t band_chain = 500, uint32_t min_seeds = 3, uint32_t min_score = 0,
                                         uint32_t band = 64, uint32_t min_depth = 3, uint32_t max_ins = 16, uint32_t min_span = 3, uint32_t min_len = 100,
                                         bool longest = false, Context &ctx = Context::global()) {
    return correct_trim_chains(read_chains<Kmer>(batch, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, ctx), batch, band, min_depth,
                               max_ins, min_span, min_len, longest, ctx);
}

// =====================================================================================================================
// string graph (kmu_sg_classify, kmu_sg_graph; the reference has no such unit)
// =====================================================================================================================

/// The thresholds of sg_classify and overlap_graph (include/kmu.h has the rules): an overlap is at least min_overlap long on both
/// reads, internal when its overhang is above max_hang or above int_permille thousandths of its length, and (with alignment
/// records) dropped below min_identity_permille; fuzz is the slack of the transitive reduction.
struct GraphParams {
    uint32_t min_overlap = 500, max_hang = 1000, int_permille = 250, min_identity_permille = 0, fuzz = 10;
};

/// What sg_classify returns: the class KMU_SG_* of every record and the summary of every read.
struct OverlapClasses {
    std::vector<uint8_t> classes;
    std::vector<kmu_sg_read> reads;
};

/// What overlap_graph returns: the arcs in (from, to, rec) order, the slice of every vertex (2r: read r forward, 2r + 1: its reverse
/// complement), and what sg_classify returns with the surviving out-degrees filled in.
struct OverlapGraph {
    std::vector<kmu_sg_arc> arcs;
    std::vector<uint64_t> arc_offsets;
    std::vector<uint8_t> classes;
    std::vector<kmu_sg_read> reads;
};

namespace detail {
inline kmu_sg_params sg_params(const GraphParams &g) {
    kmu_sg_params p{};
    p.min_overlap = g.min_overlap;
    p.max_hang = g.max_hang;
    p.int_permille = g.int_permille;
    p.min_identity_permille = g.min_identity_permille;
    p.fuzz = g.fuzz;
    return p;
}
/// the number of reads, once the offsets and the alignment records were found to fit
inline uint32_t sg_check_sizes(const char *who, const std::vector<kmu_chain> &chains, const std::vector<kmu_chain_aln> &aln, const std::vector<uint64_t> &offsets) {
    const uint32_t n_reads = n_reads_of(who, offsets);
    if (!aln.empty() && aln.size() != chains.size()) throw std::invalid_argument(std::string(who) + ": as many alignment records as chains, or none");
    return n_reads;
}
} // namespace detail

/// kmu_sg_classify on host arrays: chains of a self-join, their alignment records (empty: no identity test) and the batch's offsets.
inline OverlapClasses sg_classify(const std::vector<kmu_chain> &chains, const std::vector<kmu_chain_aln> &aln, const std::vector<uint64_t> &offsets,
                                  const GraphParams &g = GraphParams(), Context &ctx = Context::global()) {
    const uint32_t n_reads = detail::sg_check_sizes("sg_classify", chains, aln, offsets);
    OverlapClasses out;
    out.classes.assign(chains.size(), 0);
    out.reads.assign(n_reads, kmu_sg_read{});
    const kmu_sg_params p = detail::sg_params(g);
    ctx.check(kmu_sg_classify(ctx.raw(), detail::ptr(chains), detail::opt(aln), chains.size(), offsets.data(), n_reads, &p, KMU_MEM_HOST,
                              detail::ptr(out.classes), detail::ptr(out.reads)));
    return out;
}

/// kmu_sg_graph on host arrays (minimizer.overlap_graph): the dovetails between reads that are not contained as a bidirected
/// graph, transitively reduced.  Two library calls: one that counts, one with exactly that capacity.
inline OverlapGraph overlap_graph(const std::vector<kmu_chain> &chains, const std::vector<kmu_chain_aln> &aln, const std::vector<uint64_t> &offsets,
                                  const GraphParams &g = GraphParams(), Context &ctx = Context::global()) {
    const uint32_t n_reads = detail::sg_check_sizes("overlap_graph", chains, aln, offsets);
    OverlapGraph out;
    const kmu_sg_params p = detail::sg_params(g);
    using detail::ptr;
    detail::two_calls(
        ctx, true,
        [&](uint64_t total) {
            out.arcs.assign(total, kmu_sg_arc{});
            out.arc_offsets.assign(2 * size_t(n_reads) + 1, 0);
            out.classes.assign(chains.size(), 0);
            out.reads.assign(n_reads, kmu_sg_read{});
        },
        [&](bool write, uint64_t cap, uint64_t *total) {
            return kmu_sg_graph(ctx.raw(), ptr(chains), detail::opt(aln), chains.size(), offsets.data(), n_reads, &p, KMU_MEM_HOST,
                                write ? ptr(out.classes) : nullptr, write ? ptr(out.reads) : nullptr, write ? ptr(out.arcs) : nullptr, cap,
                                write ? out.arc_offsets.data() : nullptr, total);
        });
    return out;
}

/// From the reads of a batch to their string graph (minimizer.read_graph): read_alignments, then overlap_graph on its records.
template <class Kmer>
OverlapGraph read_graph(const detail::Batch &batch, size_t k, uint32_t w, const GraphParams &g = GraphParams(), FHash fhash = FHash::canon_invhash,
                        uint32_t max_occ = 0, uint32_t max_gap = 5000, uint32_t band_chain = 500, uint32_t min_seeds = 3, uint32_t min_score = 0,
                        uint32_t band = 64, Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("read_graph", batch);
    const auto records = read_alignments<Kmer>(batch, k, w, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band, ctx);
    return overlap_graph(records.first, records.second, b.offsets, g, ctx);
}

/// Which reads lie on one unitig (minimizer.unitig_labels): the components of the 2 n_reads vertices under the arcs whose `unique`
/// is 1, each unitig once per strand; a read's label is the smaller of the labels of its two vertices.
inline std::vector<uint32_t> unitig_labels(const std::vector<kmu_sg_arc> &arcs, uint32_t n_reads, Context &ctx = Context::global()) {
    static_assert(sizeof(kmu_sg_arc) == 32, "a record is 8 words");
    const Components c = detail::components_call(ctx, 2 * n_reads, [&](uint32_t *l, uint32_t *cl, uint32_t *s, uint32_t *m, uint32_t *n) {
        return kmu_components(ctx.raw(), 2 * n_reads, reinterpret_cast<const uint32_t *>(detail::ptr(arcs)), arcs.size(), 8, 6, 1, KMU_MEM_HOST, l, cl,
                              s, m, n);
    });
    std::vector<uint32_t> labels(n_reads);
    for (uint32_t r = 0; r < n_reads; r++) labels[r] = std::min(c.label[2 * size_t(r)], c.label[2 * size_t(r) + 1]);
    return labels;
}

/// One line of GFA 1 text for an arc: `L from +/- to +/- <ovl>M` (minimizer.gfa_lines writes these for the surviving arcs).
inline std::string gfa_line(const kmu_sg_arc &a, const std::string &name_from, const std::string &name_to) {
    return "L\t" + name_from + "\t" + ((a.from & 1u) ? "-" : "+") + "\t" + name_to + "\t" + ((a.to & 1u) ? "-" : "+") + "\t" + std::to_string(a.ovl) + "M";
}
/// ... and for a read: `S name * LN:i:len`
inline std::string gfa_line(const std::string &name, uint64_t len) { return "S\t" + name + "\t*\tLN:i:" + std::to_string(len); }

// =====================================================================================================================
// unitig layout (kmu_sg_unitigs, kmu_sg_unitig_seqs; the reference has no such unit)
// =====================================================================================================================

/// What sg_unitigs returns: the unitigs numbered by their smallest read, the steps (unitig u's are path[first .. first + n_reads))
/// and the place of every read (unitig KMU_SG_NONE: a contained read).
struct Unitigs {
    std::vector<kmu_sg_unitig> unitigs;
    std::vector<kmu_sg_step> path;
    std::vector<kmu_sg_place> place;
};

/// What unitig_sequences returns: the bases of all unitigs and the offset of every unitig into them.
struct UnitigSequences {
    std::vector<uint8_t> seq;
    std::vector<uint64_t> seq_offsets;
};

/// What read_unitigs returns.
struct ReadUnitigs {
    Unitigs layout;
    UnitigSequences sequences;
};

/// kmu_sg_unitigs on host arrays (minimizer.unitig_paths): the arcs whose `unique` is 1 as ordered paths of reads.  arcs, reads: of
/// overlap_graph (reads empty: no read is contained); offsets: the batch's.  One library call: both counts are at most n_reads.
inline Unitigs sg_unitigs(const std::vector<kmu_sg_arc> &arcs, const std::vector<kmu_sg_read> &reads, const std::vector<uint64_t> &offsets,
                          Context &ctx = Context::global()) {
    const uint32_t n_reads = detail::n_reads_of("sg_unitigs", offsets);
    if (!reads.empty() && reads.size() != n_reads) throw std::invalid_argument("sg_unitigs: as many summaries as reads, or none");
    Unitigs out;
    out.unitigs.assign(n_reads, kmu_sg_unitig{});
    out.path.assign(n_reads, kmu_sg_step{});
    out.place.assign(n_reads, kmu_sg_place{});
    uint64_t n_steps = 0, total = 0;
    ctx.check(kmu_sg_unitigs(ctx.raw(), detail::ptr(arcs), arcs.size(), detail::opt(reads), offsets.data(), n_reads, KMU_MEM_HOST, detail::ptr(out.unitigs),
                             detail::ptr(out.path), detail::ptr(out.place), &n_steps, &total));
    out.unitigs.resize(total);
    out.path.resize(n_steps);
    return out;
}

/// kmu_sg_unitig_seqs on host arrays (minimizer.unitig_sequences): the bases of every unitig of a layout.  Two library calls: one
/// that counts, one with exactly that capacity.
inline UnitigSequences unitig_sequences(const Unitigs &layout, const std::vector<uint8_t> &bases, const std::vector<uint64_t> &offsets,
                                        Context &ctx = Context::global()) {
    const uint32_t n_reads = detail::n_reads_of("unitig_sequences", offsets);
    using detail::ptr;
    UnitigSequences out;
    detail::two_calls(
        ctx, true, [&](uint64_t total) { out.seq.assign(total, 0), out.seq_offsets.assign(layout.unitigs.size() + 1, 0); },
        [&](bool write, uint64_t cap, uint64_t *total) {
            return kmu_sg_unitig_seqs(ctx.raw(), ptr(layout.unitigs), layout.unitigs.size(), ptr(layout.path), layout.path.size(), ptr(bases), offsets.data(),
                                      n_reads, KMU_MEM_HOST, write ? out.seq_offsets.data() : nullptr, write ? ptr(out.seq) : nullptr, cap, total);
        });
    return out;
}

/// From the reads of a batch to their unitigs and the unitigs' bases (minimizer.read_unitigs): read_graph, sg_unitigs,
/// unitig_sequences.
template <class Kmer>
ReadUnitigs read_unitigs(const detail::Batch &batch, size_t k, uint32_t w, const GraphParams &g = GraphParams(), FHash fhash = FHash::canon_invhash,
                         uint32_t max_occ = 0, uint32_t max_gap = 5000, uint32_t band_chain = 500, uint32_t min_seeds = 3, uint32_t min_score = 0,
                         uint32_t band = 64, Context &ctx = Context::global()) {
    const detail::Batch b = detail::host_batch("read_unitigs", batch);
    const OverlapGraph graph = read_graph<Kmer>(batch, k, w, g, fhash, max_occ, max_gap, band_chain, min_seeds, min_score, band, ctx);
    ReadUnitigs out;
    out.layout = sg_unitigs(graph.arcs, graph.reads, b.offsets, ctx);
    out.sequences = unitig_sequences(out.layout, b.bytes, b.offsets, ctx);
    return out;
}

/// One line of GFA text for a unitig: `S utg%06d{l|c} <seq> LN:i:<len>` (minimizer.unitig_gfa_lines), seq being its bases.
inline std::string unitig_gfa_line(uint64_t number, const kmu_sg_unitig &u, const std::string &seq) {
    char name[32];
    snprintf(name, sizeof name, "utg%06llu%c", (unsigned long long) number, (u.flags & KMU_SG_UNITIG_CIRCULAR) ? 'c' : 'l');
    return std::string("S\t") + name + "\t" + seq + "\tLN:i:" + std::to_string(u.len);
}
/// ... and for a step of it: `a <utg> <end - c> <read name> <+|-> <c>`, c = end - before being the bytes the step contributes.
inline std::string unitig_gfa_line(uint64_t number, const kmu_sg_unitig &u, const kmu_sg_step &s, uint64_t before, const std::string &read_name) {
    char name[32];
    snprintf(name, sizeof name, "utg%06llu%c", (unsigned long long) number, (u.flags & KMU_SG_UNITIG_CIRCULAR) ? 'c' : 'l');
    return std::string("a\t") + name + "\t" + std::to_string(before) + "\t" + read_name + "\t" + (s.strand ? "-" : "+") + "\t" + std::to_string(s.end - before);
}

// =====================================================================================================================
// string graph cleaning (kmu_sg_clean; the reference has no such unit)
// =====================================================================================================================

/// What sg_clean and clean_graph return: the arcs with KMU_SG_ARC_TIP / KMU_SG_ARC_BUBBLE in the flags of the removed ones and
/// `unique` recomputed, the summaries with KMU_SG_READ_TIP / KMU_SG_READ_BUBBLE and the final degrees, and the counts.
struct CleanGraph {
    std::vector<kmu_sg_arc> arcs;
    std::vector<kmu_sg_read> reads;
    kmu_sg_clean_stats stats{};
};

/// kmu_sg_clean on host arrays (Context.sg_clean): one round -- dead ends of at most max_tip_reads reads are removed, simple bubbles
/// whose branches hold at most max_bubble_reads reads are popped; 0 turns a phase off.  arcs: of overlap_graph or of an earlier
/// sg_clean, sorted by `from`; reads: the summaries (empty: none).
inline CleanGraph sg_clean(const std::vector<kmu_sg_arc> &arcs, const std::vector<kmu_sg_read> &reads, uint32_t n_reads, uint32_t max_tip_reads = 4,
                           uint32_t max_bubble_reads = 8, Context &ctx = Context::global()) {
    if (!reads.empty() && reads.size() != n_reads) throw std::invalid_argument("sg_clean: as many summaries as reads, or none");
    CleanGraph out;
    out.arcs.assign(arcs.size(), kmu_sg_arc{});
    out.reads.assign(n_reads, kmu_sg_read{});
    const kmu_sg_clean_params p{max_tip_reads, max_bubble_reads, 0u, 0u};
    ctx.check(kmu_sg_clean(ctx.raw(), detail::ptr(arcs), arcs.size(), detail::opt(reads), n_reads, &p, KMU_MEM_HOST, detail::ptr(out.arcs),
                           detail::ptr(out.reads), &out.stats));
    return out;
}

/// sg_clean repeated on its own output while a round removed something, at most `rounds` times (minimizer.clean_graph): the counts
/// are summed over the rounds, except n_arcs_left, which is the last round's.  rounds == 0 returns the inputs with zero counts.
inline CleanGraph clean_graph(const std::vector<kmu_sg_arc> &arcs, const std::vector<kmu_sg_read> &reads, uint32_t n_reads, uint32_t max_tip_reads = 4,
                              uint32_t max_bubble_reads = 8, uint32_t rounds = 1, Context &ctx = Context::global()) {
    CleanGraph out;
    out.arcs = arcs;
    out.reads = reads;
    for (uint32_t r = 0; r < rounds; r++) {
        CleanGraph next = sg_clean(out.arcs, out.reads, n_reads, max_tip_reads, max_bubble_reads, ctx);
        const kmu_sg_clean_stats s = next.stats, t = out.stats;
        next.stats = kmu_sg_clean_stats{t.n_tips + s.n_tips, t.n_tip_reads + s.n_tip_reads, t.n_spared + s.n_spared, t.n_bubbles + s.n_bubbles,
                                        t.n_bubble_reads + s.n_bubble_reads, t.n_arcs_tip + s.n_arcs_tip, t.n_arcs_bubble + s.n_arcs_bubble, s.n_arcs_left};
        out = std::move(next);
        if (!s.n_tip_reads && !s.n_bubble_reads) break;
    }
    return out;
}

/// A copy of the summaries in which every read that carries KMU_SG_READ_TIP or KMU_SG_READ_BUBBLE also carries
/// KMU_SG_READ_CONTAINED (minimizer.layout_reads): sg_unitigs then leaves the removed reads off the layout.
inline std::vector<kmu_sg_read> layout_reads(std::vector<kmu_sg_read> reads) {
    for (kmu_sg_read &r : reads)
        if (r.flags & (KMU_SG_READ_TIP | KMU_SG_READ_BUBBLE)) r.flags |= KMU_SG_READ_CONTAINED;
    return reads;
}

// =====================================================================================================================
// unitig consensus (kmu_sg_unitig_chains and the correction stages over it; the reference has no such unit)
// =====================================================================================================================

/// What sg_unitig_chains returns: at most one record per read in ascending read id -- read_a the unitig, read_b the read, score 0 for
/// a layout read and 1 for a contained one -- and the counts.
struct UnitigChains {
    std::vector<kmu_chain> records;
    kmu_um_stats stats{};
};

/// kmu_sg_unitig_chains on host arrays (Context.sg_unitig_chains): where every read lies on which unitig.  layout: of sg_unitigs;
/// chains, classes: the self-join and its classes of overlap_graph (both empty: no contained read is placed); offsets: the batch's.
inline UnitigChains sg_unitig_chains(const Unitigs &layout, const std::vector<kmu_chain> &chains, const std::vector<uint8_t> &classes,
                                     const std::vector<uint64_t> &offsets, Context &ctx = Context::global()) {
    const uint32_t n_reads = detail::n_reads_of("sg_unitig_chains", offsets);
    if (layout.place.size() != n_reads) throw std::invalid_argument("sg_unitig_chains: as many places as reads");
    if (chains.size() != classes.size()) throw std::invalid_argument("sg_unitig_chains: as many classes as chains");
    UnitigChains out;
    using detail::opt;
    using detail::ptr;
    out.records.assign(n_reads, kmu_chain{});
    const kmu_um_params p{0u, 0u};
    uint64_t total = 0;
    ctx.check(kmu_sg_unitig_chains(ctx.raw(), ptr(layout.unitigs), layout.unitigs.size(), ptr(layout.path), layout.path.size(), ptr(layout.place), opt(chains),
                                   opt(classes), chains.size(), offsets.data(), n_reads, &p, KMU_MEM_HOST, ptr(out.records), &out.stats, &total));
    out.records.resize(total);
    return out;
}
/// The same under the name of the Python route (minimizer.unitig_read_chains)
inline UnitigChains unitig_read_chains(const Unitigs &layout, const std::vector<kmu_chain> &chains, const std::vector<uint8_t> &classes,
                                       const std::vector<uint64_t> &offsets, Context &ctx = Context::global()) {
    return sg_unitig_chains(layout, chains, classes, offsets, ctx);
}

/// What polish_unitigs returns: the polished unitigs as a batch, the layout in polished coordinates (the unitigs' len and the steps'
/// end; the places are unchanged), the summaries of pile_call, and the map's records with their alignments (of the last round).
struct PolishedUnitigs {
    ConsensusReads cons;
    Unitigs layout;
    std::vector<kmu_read_pile> summaries;
    std::vector<kmu_chain> records;
    std::vector<kmu_chain_aln> aln;
    kmu_um_stats stats{};
};

/// The consensus of every unitig over its reads (minimizer.polish_unitigs): sg_unitig_chains, then -- with the unitig batch as the q
/// side and the reads as the db side -- chain_cigar, chain_pileup and chain_pile_ins with KMU_PILE_Q, pile_call with `min_depth`,
/// pile_ins_plan with `max_ins`, pile_consensus; every step's end goes into polished coordinates through pile_consensus_pos.
/// rounds > 1 translates the records' a coordinates the same way and runs the stages again on the polished batch.
inline PolishedUnitigs polish_unitigs(const Unitigs &layout, const UnitigSequences &sequences, const detail::Batch &reads,
                                      const std::vector<kmu_chain> &chains = {}, const std::vector<uint8_t> &classes = {}, uint32_t band = 64,
                                      uint64_t max_trace_bytes = 0, uint32_t min_depth = 2, uint32_t max_ins = 16, uint32_t rounds = 1,
                                      Context &ctx = Context::global()) {
    const detail::Batch db = detail::host_batch("polish_unitigs", reads);
    UnitigChains map = sg_unitig_chains(layout, chains, classes, db.offsets, ctx);
    PolishedUnitigs out;
    out.stats = map.stats;
    out.layout = layout;
    out.records = std::move(map.records);
    detail::Batch q;
    q.bytes = sequences.seq;
    q.bytes.resize(q.bytes.size() + 16, 0);
    q.offsets = sequences.seq_offsets;
    InsPlan no_slots; // the reads get no votes: a plan without slots stands for their side
    no_slots.ins_len.assign(db.offsets.back(), 0);
    for (uint32_t round = 0; round < std::max(rounds, 1u); round++) {
        const std::vector<kmu_chain> used = out.records;
        ChainCigars cigars = chain_cigar(used, q, &db, band, max_trace_bytes, ctx);
        const ChainPileups pile = chain_pileup(used, cigars, q, &db, KMU_PILE_Q, {}, ctx);
        PileCalls calls = pile_call(pile.q, q, min_depth, ctx);
        const InsPlan plan = pile_ins_plan(pile.q, calls.call, max_ins, ctx);
        const ChainInsertions ins = chain_pile_ins(used, cigars, q, plan, &db, &no_slots, KMU_PILE_Q, {}, ctx);
        out.cons = pile_consensus(pile.q, calls.call, plan, ins.q, q, ctx);
        std::vector<uint64_t> rows, base;
        auto ask = [&](uint32_t unitig, uint64_t coord) {
            rows.push_back(q.offsets[unitig] + coord);
            base.push_back(out.cons.offsets[unitig]);
        };
        for (const kmu_sg_step &s : out.layout.path) ask(out.layout.place[s.read].unitig, s.end);
        for (const kmu_chain &c : used) ask(c.read_a, c.a_start);
        for (const kmu_chain &c : used) ask(c.read_a, c.a_end);
        const std::vector<uint64_t> pos = pile_consensus_pos(pile.q, calls.call, plan, ins.q, q, rows, ctx);
        const size_t n = out.layout.path.size(), m = used.size();
        for (size_t i = 0; i < n; i++) out.layout.path[i].end = pos[i] - base[i];
        for (size_t i = 0; i < m; i++) {
            out.records[i].a_start = uint32_t(pos[n + i] - base[n + i]);
            out.records[i].a_end = uint32_t(pos[n + m + i] - base[n + m + i]);
        }
        for (size_t u = 0; u < out.layout.unitigs.size(); u++) out.layout.unitigs[u].len = out.cons.offsets[u + 1] - out.cons.offsets[u];
        out.summaries = std::move(calls.reads);
        out.aln = std::move(cigars.aln);
        if (round + 1 == std::max(rounds, 1u)) out.records = used; // the records that were aligned, as the Python route returns them
        q.bytes = out.cons.bases;
        q.bytes.resize(q.bytes.size() + 16, 0);
        q.offsets = out.cons.offsets;
    }
    return out;
}

// =====================================================================================================================
// counting (kmercount.rs)
// =====================================================================================================================

/// trait KmerCountT (kmercount.rs:48-59)
template <class Kmer> class KmerCountT {
  public:
    virtual ~KmerCountT() = default;
    virtual void insert_kmer(Kmer kmer) = 0;
    virtual uint32_t get_count(Kmer kmer) = 0;
    virtual uint64_t get_nb_distinct() = 0;
    virtual uint64_t get_nb_unique() = 0;
};

template <class Kmer> class KmerPrefilter;   // the count prefilter, below

/// KmerCounter::new(fpr, capacity, nb_bits) (kmercount.rs:70-123).  The device table is exact: the reference's contract
/// without the false positives of its cuckoo + counting-Bloom pair, so `fpr` is accepted and unused.  Single insertions
/// are queued on the host and reach the device in batches (at the latest when something is read back).
template <class Kmer> class KmerCounter : public KmerCountT<Kmer> {
  public:
    KmerCounter(double /*fpr*/, size_t capacity, uint8_t nb_bits, Context &ctx = Context::global())
        : capacity_(capacity), nb_bits_(nb_bits), ctx_(ctx) {}
    ~KmerCounter() override {
        if (counter_) kmu_count_destroy(counter_);
    }
    KmerCounter(const KmerCounter &) = delete;
    KmerCounter &operator=(const KmerCounter &) = delete;

    void insert_kmer(Kmer kmer) override {
        ensure(kmer.get_nb_base());
        pending_.push_back(uint64_t(kmer.get_compressed_value()));
        if (pending_.size() >= (size_t(1) << 20)) flush();
    }
    /// every canonical k-mer of every read: kmer.reverse_complement().min(kmer) (kmercount.rs:313, 938)
    void insert_reads(const std::vector<const Sequence *> &seqvec, uint8_t kmer_size) {
        insert_reads(detail::gather(seqvec), kmer_size);
    }
    void insert_reads(const detail::Batch &b, uint8_t kmer_size) {
        ensure(kmer_size);
        flush();
        ctx_.check(kmu_count_add_reads(counter_, b.bytes_ptr(), b.offsets_ptr(), b.packed_ptr(), b.n(), b.input_kind, b.mem()));
    }
    /// the occurrences of the reads whose k-mer the prefilter puts in class 2 (may occur twice or more); returns their number.
    /// After a filter built from the same reads every count held is exact, every k-mer seen at least twice is held, and
    /// get_nb_unique counts the singletons that slipped through the filter.
    uint64_t insert_reads_filtered(KmerPrefilter<Kmer> &filter, const detail::Batch &reads, uint8_t kmer_size) {
        const detail::Batch b = detail::unpacked(reads);   // kmu_count_add_reads_filtered takes unpacked bases
        ensure(kmer_size);
        flush();
        uint64_t passed = 0;
        ctx_.check(kmu_count_add_reads_filtered(counter_, filter.raw(), b.bytes_ptr(), b.offsets_ptr(), b.n(), b.mem(), &passed));
        return passed;
    }
    uint32_t get_count(Kmer kmer) override {
        ensure(kmer.get_nb_base());
        flush();
        const uint64_t key = kmer.get_compressed_value();
        uint32_t c = 0;
        ctx_.check(kmu_count_query(counter_, &key, 1, KMU_MEM_HOST, &c));
        return c;
    }
    std::vector<uint32_t> get_count(const std::vector<Kmer> &kmers) {
        if (kmers.empty()) return {};
        ensure(kmers[0].get_nb_base());
        flush();
        const std::vector<uint64_t> keys = detail::compressed_values(kmers);
        std::vector<uint32_t> c(keys.size());
        ctx_.check(kmu_count_query(counter_, keys.data(), keys.size(), KMU_MEM_HOST, c.data()));
        return c;
    }
    uint64_t get_nb_distinct() override {
        if (!counter_) return 0;
        flush();
        uint64_t n = 0;
        ctx_.check(kmu_count_nb_distinct(counter_, &n));
        return n;
    }
    uint64_t get_nb_unique() override {
        if (!counter_) return 0;
        flush();
        uint64_t n = 0;
        ctx_.check(kmu_count_nb_unique(counter_, &n));
        return n;
    }
    /// get_above2_count(kmer) (kmercount.rs:100-105): the count if the k-mer was seen at least twice, else 0
    uint32_t get_above2_count(Kmer kmer) {
        const uint32_t c = get_count(kmer);
        return c >= 2 ? c : 0;
    }
    /// eliminate_once_kmer (kmercount.rs:110-117): forget the k-mers seen once
    void eliminate_once_kmer() {
        if (!counter_) return;
        flush();
        ctx_.check(kmu_count_eliminate_once(counter_));
    }
    uint8_t get_count_nb_bits() const { return nb_bits_; }
    /// (canonical value, count) of the k-mers seen at least twice, sorted by value: what dump_kmer_counter writes
    std::pair<std::vector<uint64_t>, std::vector<uint32_t>> above2_entries() {
        if (!counter_) return {};
        flush();
        std::vector<uint64_t> k;
        std::vector<uint32_t> c;
        detail::two_calls(
            ctx_, true, [&](uint64_t n) { k.resize(n), c.resize(n); },
            [&](bool write, uint64_t cap, uint64_t *n) {
                return kmu_count_dump(counter_, 2, write ? detail::ptr(k) : nullptr, write ? detail::ptr(c) : nullptr, cap, n);
            });
        return {std::move(k), std::move(c)};
    }
    /// the count spectrum: hist[v] = distinct k-mers whose count (saturated at 2^nb_bits - 1) is v; hist[0] is 0
    std::vector<uint64_t> get_count_histogram() {
        std::vector<uint64_t> h(size_t(1) << nb_bits_, 0);
        if (!counter_) return h;
        flush();
        ctx_.check(kmu_count_histogram(counter_, h.data(), uint32_t(h.size()), KMU_MEM_HOST));
        return h;
    }
    /// the reads against this counter: the count of the canonical k-mer at every k-mer start (counts[offsets[i] + p], the last
    /// k - 1 positions of a read 0) and one record per read (solid: count >= solid_min)
    struct ReadsAbundance {
        std::vector<uint16_t> counts;
        std::vector<kmu_read_abundance> stats;
    };
    ReadsAbundance get_reads_abundance(const std::vector<const Sequence *> &seqvec, uint32_t solid_min = 2) {
        return get_reads_abundance(detail::gather(seqvec), solid_min);
    }
    ReadsAbundance get_reads_abundance(const detail::Batch &reads, uint32_t solid_min = 2) {
        const detail::Batch b = detail::unpacked(reads); // kmu_count_read_profile takes unpacked bases
        if (!counter_) throw KmuError(KMU_E_BAD_ARG, "get_reads_abundance: nothing has been inserted (the k-mer size is not known yet)");
        flush();
        ReadsAbundance r;
        r.counts.assign(std::max<size_t>(b.offsets.empty() ? 0 : size_t(b.offsets.back()), 1), 0);   // (without bases: one count, kept as it was)
        r.stats.assign(b.n(), kmu_read_abundance{});
        if (b.mem() != KMU_MEM_HOST) throw KmuError(KMU_E_UNSUPPORTED, "get_reads_abundance takes host-resident reads");
        ctx_.check(kmu_count_read_profile(counter_, b.bytes.data(), b.offsets.data(), b.n(), KMU_MEM_HOST, solid_min, r.counts.data(),
                                          detail::ptr(r.stats)));
        return r;
    }
    uint8_t kmer_size() const { return kmer_size_; }
    /// the device counter with everything inserted so far (null before the first insertion)
    kmu_counter *raw() {
        if (counter_) flush();
        return counter_;
    }

  private:
    void ensure(uint8_t k) {
        if (counter_) return;
        kmu_count_params p{};
        p.kmer_type = Kmer::kmu_type;
        p.kmer_size = k;
        p.counter_bits = nb_bits_;
        p.capacity_hint = capacity_;
        ctx_.check(kmu_count_create(ctx_.raw(), &p, &counter_));
        kmer_size_ = k;
    }
    void flush() {
        if (pending_.empty()) return;
        ctx_.check(kmu_count_add_kmers(counter_, pending_.data(), pending_.size(), KMU_MEM_HOST));
        pending_.clear();
    }
    size_t capacity_;
    uint8_t nb_bits_;
    Context &ctx_;
    kmu_counter *counter_ = nullptr;
    uint8_t kmer_size_ = 0;
    std::vector<uint64_t> pending_;
};

/// KmerCounterPool (kmercount.rs:424-565): upstream holds one counter per consumer thread and re-dispatches queries by
/// `intNN_hash(kmer) % n`; one GPU holds the whole key space, so the pool is one counter.
template <class Kmer> class KmerCounterPool {
  public:
    KmerCounterPool(size_t capacity, uint8_t nb_bits, Context &ctx = Context::global()) : counter_(0.03, capacity, nb_bits, ctx) {}
    uint32_t get_count(Kmer kmer) { return counter_.get_count(kmer); }
    uint64_t get_nb_distinct() { return counter_.get_nb_distinct(); }
    uint64_t get_nb_unique() { return counter_.get_nb_unique(); }
    uint32_t get_above2_count(Kmer kmer) { return counter_.get_above2_count(kmer); }   // kmercount.rs:439-444
    uint8_t get_count_nb_bits() const { return counter_.get_count_nb_bits(); }
    std::pair<std::vector<uint64_t>, std::vector<uint32_t>> above2_entries() { return counter_.above2_entries(); }
    KmerCounter<Kmer> &counter() { return counter_; }

    /// dump_kmer_counter (kmercount.rs:467-531): COUNTER_MULTIPLE u32, kmer_size u8, bytes per count u8 (= 1), number of
    /// k-mers u64, then per k-mer `Kmer::dump` + count u8.  Records come sorted by value (upstream: order of first
    /// occurrence; the order carries no meaning for a reader).  Returns the number of records.
    size_t dump_kmer_counter(const std::string &fname) {
        auto [kmers, counts] = counter_.above2_entries();
        std::ofstream out(fname, std::ios::binary);
        if (!out) throw std::runtime_error("dump_kmer_counter: cannot open " + fname);
        const uint32_t magic = COUNTER_MULTIPLE;
        const uint8_t k = counter_.kmer_size(), nbc = 1;
        const uint64_t n = kmers.size();
        out.write(reinterpret_cast<const char *>(&magic), 4);
        out.write(reinterpret_cast<const char *>(&k), 1);
        out.write(reinterpret_cast<const char *>(&nbc), 1);
        out.write(reinterpret_cast<const char *>(&n), 8);
        for (size_t i = 0; i < kmers.size(); i++) {
            if constexpr (sizeof(typename Kmer::Val) == 8) {   // Kmer64bit::dump: size byte + u64 (kmer64bit.rs:98-104)
                out.write(reinterpret_cast<const char *>(&k), 1);
                out.write(reinterpret_cast<const char *>(&kmers[i]), 8);
            } else {   // the u32 word `.0` (kmer32bit.rs:141-144)
                const uint32_t w = Kmer::build(uint32_t(kmers[i]), k).raw();
                out.write(reinterpret_cast<const char *>(&w), 4);
            }
            const uint8_t c = uint8_t(std::min<uint32_t>(counts[i], 255));
            out.write(reinterpret_cast<const char *>(&c), 1);
        }
        return kmers.size();
    }
    static constexpr uint32_t COUNTER_MULTIPLE = 0xcea2bbff;   // kmercount.rs:41

  private:
    KmerCounter<Kmer> counter_;
};

/// KmerFilter1 (kmercount.rs:985-1089): which 16-mers occur exactly once in a read set, and where.  Upstream keeps two cuckoo
/// filters (approximate, randomised per process); the exact device table answers the same questions.
class KmerFilter1 {
  public:
    struct OnceKmers {   // records of dump_in_file_once_kmer16b32bit, in file order
        std::vector<uint64_t> kmin;
        std::vector<uint32_t> numseq, numkmer;
    };
    KmerFilter1(uint8_t size, uint32_t capacity, Context &ctx = Context::global()) : counter_(0.03, capacity, 8, ctx), ctx_(ctx) {
        if (size != 16) throw std::invalid_argument("KmerFilter1 holds Kmer16b32bit");
    }
    /// insert_kmer16b32bit(kmer): the caller passes the canonical k-mer (kmercount.rs:1108-1109)
    void insert_kmer16b32bit(Kmer16b32bit kmer) { counter_.insert_kmer(kmer); }
    void insert_reads(const detail::Batch &reads) { counter_.insert_reads(reads, 16); }
    uint64_t get_nb_once() { return counter_.get_nb_unique(); }   // once_f.len()
    OnceKmers once_positions(const detail::Batch &reads) {
        const detail::Batch b = detail::unpacked(reads);   // kmu_count_once_positions takes unpacked bases
        OnceKmers r;
        kmu_counter *c = counter_.raw();
        if (!c) return r;
        uint64_t n = 0;
        ctx_.check(kmu_count_once_positions(c, b.bytes_ptr(), b.offsets_ptr(), b.n(), b.mem(), nullptr, nullptr, nullptr, 0, &n));
        r.kmin.resize(n); r.numseq.resize(n); r.numkmer.resize(n);
        if (n == 0) return r;
        if (b.on_device()) {
            DeviceBuffer dk(ctx_, n * 8), ds(ctx_, n * 4), dp(ctx_, n * 4);
            ctx_.check(kmu_count_once_positions(c, b.dev_bytes, b.dev_offsets, b.n(), KMU_MEM_DEVICE, dk.as<uint64_t>(), ds.as<uint32_t>(),
                                                dp.as<uint32_t>(), n, &n));
            dk.download(r.kmin.data(), n * 8); ds.download(r.numseq.data(), n * 4); dp.download(r.numkmer.data(), n * 4);
        } else {
            ctx_.check(kmu_count_once_positions(c, b.bytes.data(), b.offsets.data(), b.n(), KMU_MEM_HOST, r.kmin.data(),
                                                r.numseq.data(), r.numkmer.data(), n, &n));
        }
        return r;
    }
    /// dump_in_file_once_kmer16b32bit(fname, seqvec) (kmercount.rs:1031-1082): COUNTER_UNIQUE u32, kmer_size u8, number of
    /// k-mers u64, then (kmer u32, numseq u32, numkmer u32) per record.  Returns the number of k-mers dumped.
    size_t dump_in_file_once_kmer16b32bit(const std::string &fname, const detail::Batch &seqvec) {
        OnceKmers r = once_positions(seqvec);
        std::ofstream out(fname, std::ios::binary);
        if (!out) throw std::runtime_error("cannot open " + fname);
        const uint32_t magic = COUNTER_UNIQUE;
        const uint8_t k = 16;
        const uint64_t n = r.kmin.size();
        out.write(reinterpret_cast<const char *>(&magic), 4);
        out.write(reinterpret_cast<const char *>(&k), 1);
        out.write(reinterpret_cast<const char *>(&n), 8);
        for (size_t i = 0; i < r.kmin.size(); i++) {
            const uint32_t rec[3] = {uint32_t(r.kmin[i]), r.numseq[i], r.numkmer[i]};
            out.write(reinterpret_cast<const char *>(rec), 12);
        }
        return r.kmin.size();
    }
    size_t dump_in_file_once_kmer16b32bit(const std::string &fname, const std::vector<Sequence> &seqvec) {
        return dump_in_file_once_kmer16b32bit(fname, detail::gather(detail::pointers(seqvec)));
    }
    static constexpr uint32_t COUNTER_UNIQUE = 0xcea2bbdd;   // kmercount.rs:35

  private:
    KmerCounter<Kmer16b32bit> counter_;
    Context &ctx_;
};

/// filter1_kmer_16b32bit(&seqvec) -> KmerFilter1 (kmercount.rs:1093-1123)
inline std::unique_ptr<KmerFilter1> filter1_kmer_16b32bit(const std::vector<Sequence> &seqvec, Context &ctx = Context::global()) {
    uint64_t bases = 0;
    for (const Sequence &s : seqvec) bases += s.size();
    auto f = std::make_unique<KmerFilter1>(16, uint32_t(std::min<uint64_t>(std::max<uint64_t>(bases, 1024), 0xFFFFFFFFu)), ctx);
    f->insert_reads(detail::gather(detail::pointers(seqvec)));
    return f;
}

/// count_kmer_threaded_one_to_many(seqvec, nb_threads, count_size, kmer_size) -> KmerCounterPool (kmercount.rs:881-974).
/// `nb_threads` is kept for the signature (inside one GPU there is no key-space dispatch); `count_size` = bits per counter.
template <class Kmer>
std::unique_ptr<KmerCounterPool<Kmer>> count_kmer_threaded_one_to_many(const std::vector<Sequence> &seqvec, size_t /*nb_threads*/,
                                                                        size_t count_size, uint8_t kmer_size,
                                                                        Context &ctx = Context::global()) {
    uint64_t bases = 0;
    for (const Sequence &s : seqvec) bases += s.size();
    auto pool = std::make_unique<KmerCounterPool<Kmer>>(std::max<uint64_t>(bases, 1024), uint8_t(count_size), ctx);
    pool->counter().insert_reads(detail::pointers(seqvec), kmer_size);
    return pool;
}

namespace detail {
template <class Kmer> std::unique_ptr<KmerCounter<Kmer>> count_kmer(const std::vector<Sequence> &seqvec, uint8_t kmer_size, Context &ctx) {
    uint64_t bases = 0;
    for (const Sequence &s : seqvec) bases += s.size();
    // upstream sizes its filters for 1.2e9 k-mers (kmercount.rs:303); the exact table only needs the batch
    auto counter = std::make_unique<KmerCounter<Kmer>>(0.03, std::max<uint64_t>(bases, 1024), 8, ctx);
    counter->insert_reads(pointers(seqvec), kmer_size);
    return counter;
}
}  // namespace detail

/// count_kmer16b32bit(&seqvec) (kmercount.rs:332-338): every canonical 16-mer, 8-bit counts
inline std::unique_ptr<KmerCounter<Kmer16b32bit>> count_kmer16b32bit(const std::vector<Sequence> &seqvec, Context &ctx = Context::global()) {
    return detail::count_kmer<Kmer16b32bit>(seqvec, 16, ctx);
}
/// count_kmer32bit(&seqvec, kmer_size) (kmercount.rs:340-347): k <= 14
inline std::unique_ptr<KmerCounter<Kmer32bit>> count_kmer32bit(const std::vector<Sequence> &seqvec, size_t kmer_size,
                                                              Context &ctx = Context::global()) {
    if (kmer_size >= 15) throw std::invalid_argument("count_kmer32bit cannot count kmer of size greater than 14");   // panics upstream
    return detail::count_kmer<Kmer32bit>(seqvec, uint8_t(kmer_size), ctx);
}
/// count_kmer64bit(&seqvec, kmer_size) (kmercount.rs:351-362): 16 < k <= 32 upstream; k = 32 is broken there, refused here
inline std::unique_ptr<KmerCounter<Kmer64bit>> count_kmer64bit(const std::vector<Sequence> &seqvec, size_t kmer_size,
                                                              Context &ctx = Context::global()) {
    if (kmer_size > 32) throw std::invalid_argument("count_kmer64bit cannot count kmer of size greater than 32");
    if (kmer_size <= 16) throw std::invalid_argument("count_kmer64bit is too expensive, use count_kmer32bit");
    return detail::count_kmer<Kmer64bit>(seqvec, uint8_t(kmer_size), ctx);
}
/// count_kmer_thread_independant(seqvec, nb_threads, kmer_size) (kmercount.rs:797-867): upstream's other threaded driver
/// (reads split over threads, k-mers dispatched by key); one GPU holds the whole key space, so the same pool comes out
template <class Kmer>
std::unique_ptr<KmerCounterPool<Kmer>> count_kmer_thread_independant(const std::vector<Sequence> &seqvec, size_t nb_threads,
                                                                      uint8_t kmer_size, Context &ctx = Context::global()) {
    return count_kmer_threaded_one_to_many<Kmer>(seqvec, nb_threads, 8, kmer_size, ctx);
}

/// KmerPrefilter: the count prefilter (kmu_kfilter, include/kmu.h) -- a two-plane Bloom filter that tells the canonical k-mers
/// inserted once (class 1) from those that may have been inserted twice or more (class 2; 0: never inserted).  It stands where the
/// reference keeps its cuckoo filter of k-mers seen once (kmercount.rs:70-123): a first pass over the reads builds it, a second
/// pass (KmerCounter::insert_reads_filtered) counts only what may occur twice.  No k-mer inserted twice is ever missed.
template <class Kmer> class KmerPrefilter {
  public:
    KmerPrefilter(uint8_t kmer_size, uint64_t nb_cells, uint32_t nb_hashes = 4, Context &ctx = Context::global()) : ctx_(ctx) {
        kmu_kfilter_params p{};
        p.kmer_type = Kmer::kmu_type;
        p.kmer_size = kmer_size;
        p.n_hashes = nb_hashes;
        p.n_cells = nb_cells;
        ctx_.check(kmu_kfilter_create(ctx_.raw(), &p, &filter_));
    }
    ~KmerPrefilter() {
        if (filter_) kmu_kfilter_destroy(filter_);
    }
    KmerPrefilter(const KmerPrefilter &) = delete;
    KmerPrefilter &operator=(const KmerPrefilter &) = delete;

    /// cells for `expected_distinct` k-mers at `bits_per_kmer` bits each (16: 0.5 % of the singletons pass with 4 hashes)
    static uint64_t cells_for(uint64_t expected_distinct, uint32_t bits_per_kmer = 16) {
        const uint64_t n = kmu_kfilter_cells_for(expected_distinct, bits_per_kmer);
        if (n == 0) throw KmuError(KMU_E_BAD_ARG, "KmerPrefilter: more cells than a filter can have (2^32 - 1)");
        return n;
    }
    /// one occurrence of every canonical k-mer of every read
    void insert_reads(const detail::Batch &reads) {
        const detail::Batch b = detail::unpacked(reads);   // the filter takes unpacked bases
        ctx_.check(kmu_kfilter_add_reads(filter_, b.bytes_ptr(), b.offsets_ptr(), b.n(), b.mem()));
    }
    void insert_reads(const std::vector<const Sequence *> &seqvec) { insert_reads(detail::gather(seqvec)); }
    /// one occurrence of a canonical k-mer (the caller passes kmer.reverse_complement().min(kmer))
    void insert_kmer(Kmer kmer) { insert_kmer(std::vector<Kmer>{kmer}); }
    void insert_kmer(const std::vector<Kmer> &kmers) {
        const std::vector<uint64_t> keys = detail::compressed_values(kmers);
        ctx_.check(kmu_kfilter_add_kmers(filter_, keys.data(), keys.size(), KMU_MEM_HOST));
    }
    /// 0: never inserted; 1: inserted exactly once; 2: may have been inserted twice or more
    uint8_t seen_class(Kmer kmer) { return seen_class(std::vector<Kmer>{kmer})[0]; }
    std::vector<uint8_t> seen_class(const std::vector<Kmer> &kmers) {
        const std::vector<uint64_t> keys = detail::compressed_values(kmers);
        std::vector<uint8_t> cls(keys.size());
        ctx_.check(kmu_kfilter_query(filter_, keys.data(), keys.size(), KMU_MEM_HOST, cls.data()));
        return cls;
    }
    /// cells, bytes, occurrences inserted, set bits of the two planes, and the estimate of the distinct k-mers inserted
    kmu_kfilter_info_t info() {
        kmu_kfilter_info_t t{};
        ctx_.check(kmu_kfilter_info(filter_, &t));
        return t;
    }
    /// this filter becomes the filter of both inputs (same parameters): ranks that each filtered a shard
    void merge(const KmerPrefilter &other) { ctx_.check(kmu_kfilter_merge(filter_, other.filter_)); }
    /// the planes, A0 B0 A1 B1 ...
    std::vector<uint64_t> words() {
        std::vector<uint64_t> w(2 * info().n_cells);
        ctx_.check(kmu_kfilter_export(filter_, w.data(), KMU_MEM_HOST));
        return w;
    }
    /// how many k-mer occurrences of the reads are class 2: what insert_reads_filtered is going to add
    uint64_t nb_passing(const detail::Batch &reads) {
        const detail::Batch b = detail::unpacked(reads);
        uint64_t n = 0;
        ctx_.check(kmu_kfilter_select_reads(filter_, b.bytes_ptr(), b.offsets_ptr(), b.n(), b.mem(), nullptr, 0, &n));
        return n;
    }
    kmu_kfilter *raw() const { return filter_; }

  private:
    Context &ctx_;
    kmu_kfilter *filter_ = nullptr;
};

/// what count_repeated_kmers returns: the counter of the k-mers that passed, the filter, and the occurrences that passed
template <class Kmer> struct RepeatedKmers {
    std::unique_ptr<KmerCounterPool<Kmer>> counter;
    std::unique_ptr<KmerPrefilter<Kmer>> filter;
    uint64_t nb_passed = 0;
};

/// count_repeated_kmers(reads, kmer_size, count_size, bits_per_kmer, nb_hashes, capacity): the counts of the k-mers seen at least
/// twice without a table slot for (nearly) every singleton.  Two passes over the reads: the filter, sized from the number of k-mer
/// occurrences, then the table, which gets the occurrences of class-2 k-mers only.  Every count held is exact and every k-mer seen
/// at least twice is held, so get_above2_count and dump_kmer_counter answer as after count_kmer_threaded_one_to_many; a k-mer that
/// is absent occurred 0 or 1 times, and get_nb_unique counts the singletons that slipped through the filter.  capacity 0: the
/// number P of passing occurrences, which can never overflow (R repeated and F slipped k-mers need P >= 2 R + F >= R + F); a
/// caller may pass something tighter from info().est_distinct - (info().n_added - P).
template <class Kmer>
RepeatedKmers<Kmer> count_repeated_kmers(const detail::Batch &reads, uint8_t kmer_size, size_t count_size = 8, uint32_t bits_per_kmer = 16,
                                         uint32_t nb_hashes = 4, uint64_t capacity = 0, Context &ctx = Context::global()) {
    const detail::Batch b = detail::unpacked(reads);
    uint64_t occurrences = 0;
    for (uint32_t i = 0; i < b.n(); i++) {
        const uint64_t len = b.offsets[i + 1] - b.offsets[i];
        if (len >= kmer_size) occurrences += len - kmer_size + 1;
    }
    RepeatedKmers<Kmer> r;
    r.filter = std::make_unique<KmerPrefilter<Kmer>>(kmer_size, KmerPrefilter<Kmer>::cells_for(occurrences, bits_per_kmer), nb_hashes, ctx);
    r.filter->insert_reads(b);
    const uint64_t passing = r.filter->nb_passing(b);
    r.counter = std::make_unique<KmerCounterPool<Kmer>>(std::max<uint64_t>(capacity ? capacity : passing, 1024), uint8_t(count_size), ctx);
    r.nb_passed = r.counter->counter().insert_reads_filtered(*r.filter, b, kmer_size);
    return r;
}
template <class Kmer>
RepeatedKmers<Kmer> count_repeated_kmers(const std::vector<Sequence> &seqvec, uint8_t kmer_size, size_t count_size = 8,
                                         uint32_t bits_per_kmer = 16, uint32_t nb_hashes = 4, uint64_t capacity = 0,
                                         Context &ctx = Context::global()) {
    return count_repeated_kmers<Kmer>(detail::gather(detail::pointers(seqvec)), kmer_size, count_size, bits_per_kmer, nb_hashes, capacity, ctx);
}

/// KmerCountReload (kmercount.rs:1132-1500): a dump of the counter read back -- for up-to-32-bit k-mers, as upstream
struct KmerCoord {   // kmercount.rs: read_num, pos
    uint32_t read_num, pos;
};
enum class CounterType { Unique, Multiple };
class KmerCountReload {
  public:
    uint32_t get_kmer_size() const { return kmer_size_; }
    size_t get_nb_kmer() const { return nb_kmer_; }
    /// get_coord_from_rank (kmercount.rs:1479-1486)
    std::optional<KmerCoord> get_coord_from_rank(size_t rank) const {
        if (rank < positions_.size()) return positions_[rank];
        return std::nullopt;
    }
    /// get_multi_kmer_counts (kmercount.rs:1489-1500): here in file order
    std::optional<std::vector<uint16_t>> get_multi_kmer_counts() const {
        if (type_ != CounterType::Multiple) return std::nullopt;
        return counts_;
    }
    const std::vector<uint32_t> &kmers() const { return kmers_; }   // the u32 words as dumped (Kmer32bit carries k in its top nibble)
    /// load_multiple_kmers_from_file (kmercount.rs:1209-1351): COUNTER_MULTIPLE, kmer_size u8, bytes per count u8, number u64,
    /// then (kmer u32, count) until the end of the file (upstream's header count is approximate, :1200-1207)
    static std::unique_ptr<KmerCountReload> load_multiple_kmers_from_file(const std::string &fname) {
        std::ifstream in(fname, std::ios::binary);
        uint32_t magic = 0;
        uint8_t k = 0, nbc = 0;
        uint64_t n = 0;
        in.read(reinterpret_cast<char *>(&magic), 4); in.read(reinterpret_cast<char *>(&k), 1);
        in.read(reinterpret_cast<char *>(&nbc), 1); in.read(reinterpret_cast<char *>(&n), 8);
        if (!in || magic != 0xcea2bbff || (nbc != 1 && nbc != 2) || k > 16) return nullptr;
        auto r = std::unique_ptr<KmerCountReload>(new KmerCountReload(CounterType::Multiple, k, n));
        for (;;) {
            uint32_t kmer = 0;
            uint16_t c = 0;
            in.read(reinterpret_cast<char *>(&kmer), 4);
            in.read(reinterpret_cast<char *>(&c), nbc);
            if (!in) break;
            r->kmers_.push_back(kmer);
            r->counts_.push_back(c);
        }
        return r;
    }
    /// load_unique_kmer_from_file (kmercount.rs:1356-1470): COUNTER_UNIQUE, kmer_size u8, number u64, then (kmer u32, numseq u32,
    /// numkmer u32)
    static std::unique_ptr<KmerCountReload> load_unique_kmer_from_file(const std::string &fname) {
        std::ifstream in(fname, std::ios::binary);
        uint32_t magic = 0;
        uint8_t k = 0;
        uint64_t n = 0;
        in.read(reinterpret_cast<char *>(&magic), 4); in.read(reinterpret_cast<char *>(&k), 1); in.read(reinterpret_cast<char *>(&n), 8);
        if (!in || magic != 0xcea2bbdd) return nullptr;
        auto r = std::unique_ptr<KmerCountReload>(new KmerCountReload(CounterType::Unique, k, n));
        for (;;) {
            uint32_t rec[3];
            in.read(reinterpret_cast<char *>(rec), 12);
            if (!in) break;
            r->kmers_.push_back(rec[0]);
            r->positions_.push_back(KmerCoord{rec[1], rec[2]});
        }
        return r;
    }

  private:
    KmerCountReload(CounterType t, uint32_t k, size_t n) : type_(t), kmer_size_(k), nb_kmer_(n) {}
    CounterType type_;
    uint32_t kmer_size_;
    size_t nb_kmer_;
    std::vector<uint32_t> kmers_;
    std::vector<KmerCoord> positions_;
    std::vector<uint16_t> counts_;
};

// =====================================================================================================================
// io: the reader rule of datasketcher / parsefastq, on the device
// =====================================================================================================================

/// Accepted reads of a FASTQ text as one byte array + offsets (the form every kernel consumes), plus the reader's tallies
/// (io.rs:37-57, datasketcher.rs:358-388: a record with a byte outside ACGTacgt is dropped and counted).
struct FastqReads {
    std::vector<uint8_t> bases;
    std::vector<uint64_t> offsets;
    kmu_ingest_info info{};
    size_t nb_reads() const { return offsets.empty() ? 0 : offsets.size() - 1; }
};

/// reads [first, last) as a batch for the sketchers / the counter
inline detail::Batch batch_of(const FastqReads &r, size_t first, size_t last) {
    detail::Batch b;
    b.offsets.resize(last - first + 1);
    for (size_t i = first; i <= last; i++) b.offsets[i - first] = r.offsets[i] - r.offsets[first];
    b.bytes.assign(r.bases.begin() + r.offsets[first], r.bases.begin() + r.offsets[last]);
    b.bytes.resize(b.bytes.size() + 16, 0);
    return b;
}

/// FASTQ or FASTA by the first byte, like needletail::parse_fastx_file (io.rs:37)
inline FastqReads parse_fastx_text(const uint8_t *text, size_t n, Context &ctx = Context::global()) {
    FastqReads r;
    ctx.check(kmu_ingest_fastx(ctx.raw(), text, n, KMU_MEM_HOST, nullptr, 0, nullptr, 0, nullptr, &r.info));
    r.bases.resize(r.info.kept_bases + 16);
    r.offsets.resize(r.info.n_kept + 1);
    ctx.check(kmu_ingest_fastx(ctx.raw(), text, n, KMU_MEM_HOST, r.bases.data(), r.bases.size(), r.offsets.data(),
                               r.offsets.size(), nullptr, &r.info));
    return r;
}
inline FastqReads parse_fastq_text(const uint8_t *text, size_t n, Context &ctx = Context::global()) {
    return parse_fastx_text(text, n, ctx);
}

/// The same, with the accepted reads LEFT ON THE DEVICE: the file's text goes up once, the reads never come back --
/// sketchers and counters take ranges of them (`batch(first, last)`) and only signatures / counts cross PCIe.
class DeviceReads {
  public:
    kmu_ingest_info info{};
    std::vector<uint64_t> offsets;   // host copy (n + 1): sizes, pack boundaries, block layouts
    size_t nb_reads() const { return offsets.empty() ? 0 : offsets.size() - 1; }
    /// reads [first, last): no copy, the device offsets index the whole base array
    detail::Batch batch(size_t first, size_t last) const {
        detail::Batch b;
        b.offsets.assign(offsets.begin() + first, offsets.begin() + last + 1);
        b.dev_bytes = bases_.as<uint8_t>();
        b.dev_offsets = offsets_dev_.as<uint64_t>() + first;
        return b;
    }
    /// whether the quality lines were kept (a FASTQ text read with_quals), and then the raw quality bytes of reads [first, last)
    /// laid out as their bases are
    bool has_quals() const { return quals_.data() != nullptr; }
    detail::Batch quals_batch(size_t first, size_t last) const {
        detail::Batch b = batch(first, last);
        b.dev_bytes = quals_.as<uint8_t>();
        return b;
    }
    /// from_device_text that keeps the quality lines of a FASTQ text on the device too (kmu_ingest_fastq_qual); a FASTA text has none
    static DeviceReads from_device_text_qual(Context &ctx, const uint8_t *d_text, uint64_t n) {
        uint8_t first = 0;
        if (n) ctx.check(kmu_copy_to_host(ctx.raw(), &first, d_text, 1));
        if (first != '@') return from_device_text(ctx, d_text, n);
        DeviceReads r;
        ctx.check(kmu_ingest_fastq_qual(ctx.raw(), d_text, n, KMU_MEM_DEVICE, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, &r.info));
        r.bases_ = DeviceBuffer(ctx, r.info.kept_bases + 64);
        r.quals_ = DeviceBuffer(ctx, r.info.kept_bases + 64);
        r.offsets_dev_ = DeviceBuffer(ctx, (r.info.n_kept + 1) * 8);
        ctx.check(kmu_ingest_fastq_qual(ctx.raw(), d_text, n, KMU_MEM_DEVICE, r.bases_.as<uint8_t>(), r.bases_.bytes(), r.quals_.as<uint8_t>(),
                                        r.quals_.bytes(), r.offsets_dev_.as<uint64_t>(), r.info.n_kept + 1, nullptr, &r.info));
        r.offsets.resize(r.info.n_kept + 1);
        r.offsets_dev_.download(r.offsets.data(), r.offsets.size() * 8);
        return r;
    }
    /// FASTQ / FASTA text already on the device (16-byte aligned) -> accepted reads on the device
    static DeviceReads from_device_text(Context &ctx, const uint8_t *d_text, uint64_t n) {
        DeviceReads r;
        ctx.check(kmu_ingest_fastx(ctx.raw(), d_text, n, KMU_MEM_DEVICE, nullptr, 0, nullptr, 0, nullptr, &r.info));
        r.bases_ = DeviceBuffer(ctx, r.info.kept_bases + 64);
        r.offsets_dev_ = DeviceBuffer(ctx, (r.info.n_kept + 1) * 8);
        ctx.check(kmu_ingest_fastx(ctx.raw(), d_text, n, KMU_MEM_DEVICE, r.bases_.as<uint8_t>(), r.bases_.bytes(),
                                   r.offsets_dev_.as<uint64_t>(), r.info.n_kept + 1, nullptr, &r.info));
        r.offsets.resize(r.info.n_kept + 1);
        r.offsets_dev_.download(r.offsets.data(), r.offsets.size() * 8);
        return r;
    }
    /// The file goes up in slabs: `n_readers` threads read slabs of it in parallel (pread), each slab is uploaded as soon
    /// as it is in memory (uploads are serialised: one context, one thread at a time), so reading and PCIe overlap.
    static DeviceReads from_file(const std::string &fname, Context &ctx = Context::global(), size_t slab = size_t(64) << 20,
                                 unsigned n_readers = 4) {
        uint64_t n = 0;
        const DeviceBuffer text = upload_file(fname, ctx, slab, n_readers, &n);
        return from_device_text(ctx, text.as<uint8_t>(), n);
    }
    /// from_file through from_device_text_qual
    static DeviceReads from_file_qual(const std::string &fname, Context &ctx = Context::global(), size_t slab = size_t(64) << 20,
                                      unsigned n_readers = 4) {
        uint64_t n = 0;
        const DeviceBuffer text = upload_file(fname, ctx, slab, n_readers, &n);
        return from_device_text_qual(ctx, text.as<uint8_t>(), n);
    }

  private:
    /// the text of a file in a device buffer, *n_out its size
    static DeviceBuffer upload_file(const std::string &fname, Context &ctx, size_t slab, unsigned n_readers, uint64_t *n_out) {
        const int fd = ::open(fname.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("cannot open " + fname);
        struct stat st;
        if (::fstat(fd, &st) != 0) {
            ::close(fd);
            throw std::runtime_error("cannot stat " + fname);
        }
        const uint64_t n = uint64_t(st.st_size);
        DeviceBuffer text(ctx, n + 64);
        const uint64_t n_slabs = (n + slab - 1) / slab;
        std::atomic<uint64_t> next{0};
        std::mutex upload_lock;
        std::string error;
        auto reader = [&]() {
            std::vector<char> host(std::min<uint64_t>(slab, std::max<uint64_t>(n, 1)));
            for (;;) {
                const uint64_t i = next.fetch_add(1);
                if (i >= n_slabs) return;
                const uint64_t at = i * slab, want = std::min<uint64_t>(slab, n - at);
                uint64_t got = 0;
                while (got < want) {
                    const ssize_t r = ::pread(fd, host.data() + got, want - got, off_t(at + got));
                    if (r <= 0) break;
                    got += uint64_t(r);
                }
                std::lock_guard<std::mutex> g(upload_lock);
                if (got != want) {
                    error = "short read on " + fname;
                    next = n_slabs;
                    return;
                }
                try {
                    text.upload(host.data(), want, at);
                } catch (const std::exception &e) {
                    error = e.what();
                    next = n_slabs;
                    return;
                }
            }
        };
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < std::max(1u, n_readers) && t < n_slabs; t++) pool.emplace_back(reader);
        reader();
        for (auto &t : pool) t.join();
        ::close(fd);
        if (!error.empty()) throw std::runtime_error(error);
        *n_out = n;
        return text;
    }
    DeviceBuffer bases_, offsets_dev_, quals_;
};

inline FastqReads parse_fastq_file(const std::string &fname, Context &ctx = Context::global()) {
    std::ifstream in(fname, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error("cannot open " + fname);
    const std::streamsize n = in.tellg();
    in.seekg(0);
    std::vector<uint8_t> text(size_t(n) + 16);
    in.read(reinterpret_cast<char *>(text.data()), n);
    return parse_fastq_text(text.data(), size_t(n), ctx);
}

// =====================================================================================================================
// statutils + quality: the base and quality distributions of a read set, on the device (kmu_read_stats.hip)
// =====================================================================================================================

/// a double as Rust's `{}` prints it: the shortest decimal that reads back to the same value, never an exponent, no `.0`
inline std::string rust_display(double x) {
    if (std::isnan(x)) return "NaN";
    if (std::isinf(x)) return x > 0 ? "inf" : "-inf";
    char buf[400];
    const std::to_chars_result r = std::to_chars(buf, buf + sizeof buf, x, std::chars_format::fixed);
    return std::string(buf, r.ptr);
}

/// statutils.rs:38-50.  acgt_distribution: [101][4] row-major, the reads whose base (column A C G T) sits at a percentage (row) over
/// the number of reads.  The read sizes are the counts of the length buckets of (maxreadlen, prec) -- HdrHistogram's layout,
/// include/kmu.h -- with histo_out the reads beyond them; non_acgt the bytes that are no base.
/// value_at_quantile is written from that layout; the hdrhistogram crate's source was not at hand to check its rule to the letter, so
/// readlen.histo is NOT claimed to be byte for byte the reference's (bases.histo has no such caveat).
class ReadBaseDistribution {
  public:
    std::vector<double> acgt_distribution;
    std::vector<uint64_t> len_hist;
    uint64_t nb_reads = 0, upper_histo = 0, histo_out = 0, non_acgt = 0;
    int prec = 3;

    ReadBaseDistribution(const std::vector<uint64_t> &pct_hist, std::vector<uint64_t> len_hist_, uint64_t nb_reads_, uint64_t histo_out_,
                         uint64_t non_acgt_, uint64_t maxreadlen, int prec_)
        : acgt_distribution(pct_hist.size()), len_hist(std::move(len_hist_)), nb_reads(nb_reads_), upper_histo(maxreadlen), histo_out(histo_out_),
          non_acgt(non_acgt_), prec(prec_ > 5 ? 5 : prec_) {
        const double inv = 1. / double(nb_reads);   // (statutils.rs:333: the table times the inverse)
        for (size_t i = 0; i < pct_hist.size(); i++) acgt_distribution[i] = double(pct_hist[i]) * inv;
    }
    /// Histogram::len(): the number of recorded lengths
    uint64_t readsize_len() const {
        uint64_t n = 0;
        for (uint64_t c : len_hist) n += c;
        return n;
    }
    /// the highest length of the first bucket whose running count reaches max(1, ceil(q * recorded)); 0 for an empty histogram
    uint64_t value_at_quantile(double q) const {
        const uint64_t total = readsize_len();
        if (total == 0) return 0;
        const uint64_t need = std::max<uint64_t>(1, std::min<uint64_t>(total, uint64_t(std::ceil(std::min(q, 1.0) * double(total)))));
        uint64_t running = 0, lowest = 0, highest = 0;
        for (size_t b = 0; b < len_hist.size(); b++) {
            running += len_hist[b];
            if (running >= need) {
                if (kmu_len_bucket_range(prec, uint32_t(b), &lowest, &highest) != KMU_OK) throw std::invalid_argument("value_at_quantile: bad precision");
                return highest;
            }
        }
        return highest;
    }
    /// 101 lines `a c  g  t ` (statutils.rs:96-103)
    void ascii_dump_acgt_distribution(const std::string &name) const {
        std::ofstream f(name, std::ios::trunc);
        if (!f) throw std::runtime_error("could not open file " + name);
        for (size_t i = 0; i + 3 < acgt_distribution.size(); i += 4)
            f << rust_display(acgt_distribution[i]) << " " << rust_display(acgt_distribution[i + 1]) << "  " << rust_display(acgt_distribution[i + 2])
              << "  " << rust_display(acgt_distribution[i + 3]) << " \n";
    }
    /// statutils.rs:118-190, step by step: `readsize  nb reads ` lines at regular quantiles.  A histogram of fewer than 100 entries
    /// is refused: nothing is written and the error text is returned (empty otherwise).
    std::string ascii_dump_readlen_distribution(const std::string &name) const {
        const uint64_t nb_entries = readsize_len();
        if (nb_entries == 0) return "histogram error!, empty histogram";
        const uint64_t maxlen = nb_entries;   // (statutils.rs:127: the number of entries, not a length)
        std::printf("ascii_dump_readlen_distribution nb_entries %llu  maxlen %llu\n", (unsigned long long) nb_entries, (unsigned long long) maxlen);
        if (nb_entries < 100) {
            std::printf("Error : ascii_dump_readlen_distribution nb_entries too small : %llu\n", (unsigned long long) nb_entries);
            return "histogram error!";
        }
        const uint64_t nbslot = nb_entries / 100;
        std::vector<uint64_t> readsize(nbslot + 1);
        for (uint64_t i = 0; i <= nbslot; i++) readsize[i] = value_at_quantile(double(i) / double(nbslot));
        const uint64_t nb_points = 1000;
        std::vector<std::pair<uint64_t, uint64_t>> points;
        uint64_t first_i = 0, current_i = 0;
        for (uint64_t j = 0; j < nb_points; j++) {
            const uint64_t threshold = (maxlen * j) / nb_points;
            while (readsize[current_i] < threshold && current_i < nbslot) current_i++;
            if (current_i < nbslot && current_i > first_i) points.emplace_back(readsize[current_i], ((current_i - first_i) * nb_entries) / nbslot);
            first_i = current_i;
        }
        std::ofstream f(name, std::ios::trunc);
        if (!f) return "could not open file " + name;
        for (const auto &pt : points) f << pt.first << "  " << pt.second << " \n";
        return "";
    }
};

/// statutils.rs:276-347 on the device: the reads of a batch, in host memory or left on the device by DeviceReads.  (The reference
/// also writes `bases.histo` into the working directory here; the caller does that, where it wants the file.)
inline ReadBaseDistribution get_base_count_par(const detail::Batch &reads, uint64_t maxreadlen, uint8_t prec, Context &ctx = Context::global()) {
    const detail::Batch b = detail::unpacked(reads);
    kmu_read_stats_params p{};
    p.sig_digits = prec > 5 ? 5 : prec;
    p.max_len = maxreadlen;
    uint32_t n_buckets = 0;
    uint64_t limit = 0;
    if (kmu_len_hist_layout(p.max_len, p.sig_digits, &n_buckets, &limit) != KMU_OK)
        throw std::invalid_argument("get_base_count_par: maxreadlen must be positive and prec at least 1");
    std::vector<uint64_t> pct(101 * 4), hist(n_buckets);
    kmu_read_stats_info info{};
    if (b.on_device()) {
        DeviceBuffer d_pct(ctx, pct.size() * 8), d_hist(ctx, hist.size() * 8);
        ctx.check(kmu_read_stats(ctx.raw(), &p, b.bytes_ptr(), b.offsets_ptr(), b.n(), KMU_MEM_DEVICE, nullptr, d_pct.as<uint64_t>(),
                                 d_hist.as<uint64_t>(), &info));
        d_pct.download(pct.data(), pct.size() * 8);
        d_hist.download(hist.data(), hist.size() * 8);
    } else {
        ctx.check(kmu_read_stats(ctx.raw(), &p, detail::ptr(b.bytes), b.offsets.data(), b.n(), KMU_MEM_HOST, nullptr, pct.data(), hist.data(), &info));
    }
    return ReadBaseDistribution(pct, std::move(hist), info.n_reads, info.histo_out, info.n_other, maxreadlen, p.sig_digits);
}

/// quality.rs:33-43 in integers: 0 below 0x25, then one class per three values, 7 from 0x37 on
inline uint8_t remap_quality8(uint8_t q) { return q < 0x25 ? uint8_t(0) : uint8_t(std::min(7, 1 + (int(q) - 0x25) / 3)); }

/// FastqReads with the raw quality byte of every base: quals[offsets[i] + p] belongs to base p of kept read i
struct FastqQualReads : FastqReads {
    std::vector<uint8_t> quals;
};
/// kmu_ingest_fastq_qual on a host text: the reads kmu_ingest_fastq keeps, and their quality lines
inline FastqQualReads ingest_fastq_qual(const uint8_t *text, size_t n, Context &ctx = Context::global()) {
    FastqQualReads r;
    ctx.check(kmu_ingest_fastq_qual(ctx.raw(), text, n, KMU_MEM_HOST, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, &r.info));
    r.bases.resize(r.info.kept_bases + 16);
    r.quals.resize(r.info.kept_bases + 16);
    r.offsets.resize(r.info.n_kept + 1);
    ctx.check(kmu_ingest_fastq_qual(ctx.raw(), text, n, KMU_MEM_HOST, r.bases.data(), r.bases.size(), r.quals.data(), r.quals.size(),
                                    r.offsets.data(), r.offsets.size(), nullptr, &r.info));
    return r;
}

/// kmu_read_qual_stats: one record per read and the bases of the batch per quality class
struct ReadQualityStats {
    std::vector<kmu_read_qual> reads;
    std::array<uint64_t, 8> class_hist{};
};
/// of a batch whose bytes are raw qualities (DeviceReads::quals_batch, or host arrays); want_reads false: the class totals alone
inline ReadQualityStats read_quality_stats(const detail::Batch &quals, bool want_reads = true, Context &ctx = Context::global()) {
    ReadQualityStats r;
    if (want_reads) r.reads.resize(quals.n());
    if (quals.on_device()) {
        DeviceBuffer d_reads(ctx, std::max<uint64_t>(r.reads.size() * sizeof(kmu_read_qual), 16)), d_hist(ctx, 64);
        ctx.check(kmu_read_qual_stats(ctx.raw(), quals.bytes_ptr(), quals.offsets_ptr(), quals.n(), KMU_MEM_DEVICE,
                                      want_reads ? d_reads.as<kmu_read_qual>() : nullptr, d_hist.as<uint64_t>()));
        if (!r.reads.empty()) d_reads.download(r.reads.data(), r.reads.size() * sizeof(kmu_read_qual));
        d_hist.download(r.class_hist.data(), 64);
    } else {
        ctx.check(kmu_read_qual_stats(ctx.raw(), detail::ptr(quals.bytes), quals.offsets.data(), quals.n(), KMU_MEM_HOST,
                                      want_reads ? detail::ptr(r.reads) : nullptr, r.class_hist.data()));
    }
    return r;
}
inline ReadQualityStats read_quality_stats(const std::vector<uint8_t> &quals, const std::vector<uint64_t> &offsets, Context &ctx = Context::global()) {
    detail::Batch b;
    b.bytes = quals;
    b.offsets = offsets;
    detail::n_reads_of("read_quality_stats", offsets);
    return read_quality_stats(b, true, ctx);
}

}  // namespace kmerutils

#endif  // KMERUTILS_HPP

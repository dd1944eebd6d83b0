// test_anchor -- gen_read_anchors of the C++ mirror (include/kmerutils.hpp) against the oracle: every slice of three reads is
// the oracle's bottom-k row of the bases [beg, end) handed over as a sequence of their own.  Without a device it stops with the
// library's error ("no CPU fallback"): nothing is computed on the host.
#include <cstdio>
#include <sstream>
#include <string>

#include "../../include/kmerutils.hpp"
#include "../../oracle/kmu_oracle.h"

using namespace kmerutils;

namespace {

struct Failure : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) {                                                                                                \
            std::ostringstream os_;                                                                                   \
            os_ << __FILE__ << ":" << __LINE__ << ": " #cond;                                                         \
            throw Failure(os_.str());                                                                                 \
        }                                                                                                             \
    } while (0)

std::string random_read(uint64_t &state, size_t len) {
    std::string s(len, 'A');
    for (char &c : s) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        c = "ACGT"[(state >> 33) & 3];
    }
    return s;
}

void test_gen_read_anchors() {
    const uint32_t window = 400, overlap = 100, stride = window - overlap, nbkmer = 16;
    const int k = 21;
    uint64_t state = 0xA5C3;
    // 2 * stride + 1 bases: the last slice is empty (beg == end); 1037: an odd length; 250: shorter than the window
    const std::vector<size_t> lens = {2 * stride + 1, 1037, 250};
    std::vector<std::string> reads;
    std::vector<Sequence> seqs;
    for (size_t len : lens) {
        reads.push_back(random_read(state, len));
        seqs.emplace_back(std::string_view(reads.back()));
    }
    const AnchorsGeneratorParameters params("reads.fasta", window, nbkmer, uint16_t(k), overlap);
    CHECK(params.get_window() == window && params.get_nbkmer() == nbkmer && params.get_kmer_size() == k &&
          params.get_overlap() == overlap && params.get_fasta_name() == "reads.fasta");
    const auto anchors = gen_read_anchors<Kmer64bit>(params, 7, detail::pointers(seqs));
    CHECK(anchors.size() == reads.size());
    kmu_sketch_params p{};
    p.algo = KMU_ALGO_BOTTOMK; p.kmer_type = KMU_KMER64BIT; p.kmer_size = k; p.sketch_size = int32_t(nbkmer);
    p.sig_type = KMU_SIG_U64; p.hasher = KMU_HASHER_INT64HASH; p.fhash = KMU_FHASH_VALUE_MASKED; p.input_kind = KMU_INPUT_ASCII;
    for (size_t i = 0; i < reads.size(); i++) {
        const size_t L = reads[i].size();
        CHECK(anchors[i].readnum == 7 + i);
        CHECK(anchors[i].get_nb_slice() == (L + stride - 1) / stride);
        for (size_t s = 0; s < anchors[i].get_nb_slice(); s++) {
            const SliceAnchor<Kmer64bit> &a = anchors[i].anchors[s];
            const size_t beg = s * stride, end = std::min<size_t>(beg + window, L - 1);
            CHECK(a.readnum == 7 + i && a.slicepos == beg);
            std::vector<uint8_t> sub(reads[i].begin() + beg, reads[i].begin() + end);
            const uint64_t off[2] = {0, sub.size()};
            sub.resize(sub.size() + 16);
            std::vector<uint64_t> h(nbkmer, UINT64_MAX);
            std::vector<uint32_t> c(nbkmer, 0);
            if (end > beg) { // (the oracle, like the reference, has no row for an empty sequence)
                const int rc = kmo_sketch(&p, sub.data(), off, nullptr, 1, nullptr, h.data(), c.data());
                if (rc) throw Failure("oracle kmo_sketch failed: " + std::to_string(rc));
            }
            size_t n = 0;
            while (n < nbkmer && h[n] != UINT64_MAX) n++;
            CHECK(a.minhash.size() == n);
            for (size_t t = 0; t < n; t++) CHECK(a.minhash[t].hashed == h[t] && a.minhash[t].count == c[t]);
            if (n) CHECK(a.get_minhash_key() == h[0]);
        }
    }
    CHECK(anchors[0].anchors.back().minhash.empty()); // L = 1 (mod stride): the reference panics there, here an empty slice
}

}  // namespace

int main() {
    try {
        test_gen_read_anchors();
        std::printf("ok test_gen_read_anchors\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_gen_read_anchors: %s\n", e.what());
        return 1;
    }
}

// test_syncmers -- read_syncmers of the C++ mirror (include/kmerutils.hpp) against the rule written out as a plain loop over the
// mirror's own kmer_hashes: the k-mer at p is selected iff g(p + t) or g(p + u - t) equals the smallest g over [p, p + u], u = k - s,
// g the hashes of the s-mers.  Reads with 1, 2, TILE - 1, TILE, TILE + 1, 2 TILE, 2 TILE + 1 and 5 TILE + 3 k-mers.  Without a
// device it stops with the library's error ("no CPU fallback"): nothing is computed on the host.
#include <cstdio>
#include <sstream>
#include <string>

#include "../../include/kmerutils.hpp"

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

// SKmer: the type the s-mers are hashed as (syncmer_s_type(s) names the same one)
template <class SKmer> void check_against_the_loop(const std::vector<std::string> &reads, size_t k, size_t s, uint32_t t, FHash fhash) {
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    const detail::Batch b = detail::gather(detail::pointers(seqs));
    CHECK(SKmer::kmu_type == syncmer_s_type(s));
    const std::vector<uint64_t> h = kmer_hashes<Kmer64bit>(b, k, fhash);
    const std::vector<uint64_t> g = kmer_hashes<SKmer>(b, s, fhash);
    const std::vector<uint64_t> h_fwd = kmer_hashes<Kmer64bit>(b, k, FHash::value_masked);
    const std::vector<uint64_t> h_can = kmer_hashes<Kmer64bit>(b, k, FHash::canon_value);
    const Minimizers m = read_syncmers<Kmer64bit>(b, k, s, t, fhash);
    const bool canonical = fhash == FHash::canon_invhash || fhash == FHash::canon_value || fhash == FHash::canon_raw;
    const uint64_t u = k - s;
    CHECK(m.offsets.size() == reads.size() + 1 && m.offsets[0] == 0 && m.offsets.back() == m.size());
    CHECK(m.pos.size() == m.size() && m.read.size() == m.size() && m.strand.size() == m.size());
    for (size_t i = 0; i < reads.size(); i++) {
        const uint64_t L = reads[i].size(), nk = L >= k ? L - k + 1 : 0, at = b.offsets[i];
        uint64_t e = m.offsets[i];
        for (uint64_t p = 0; p < nk; p++) {
            uint64_t least = g[at + p];
            for (uint64_t q = p; q <= p + u; q++) least = std::min(least, g[at + q]);
            if (g[at + p + t] != least && g[at + p + u - t] != least) continue;
            CHECK(e < m.offsets[i + 1]);
            CHECK(m.pos[e] == p && m.read[e] == i && m.hashes[e] == h[at + p]);
            CHECK(m.strand[e] == (canonical && h_can[at + p] != h_fwd[at + p] ? 1 : 0));
            e++;
        }
        CHECK(e == m.offsets[i + 1]);
    }
}

void test_read_syncmers() {
    uint64_t state = 0x5EED;
    const size_t k = 21, T = KMU_SYNCMER_TILE;
    std::vector<std::string> reads;
    for (size_t nk : {size_t(1), size_t(2), T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3}) reads.push_back(random_read(state, nk + k - 1));
    reads.push_back(random_read(state, 17)); // shorter than k
    reads.push_back(std::string());
    check_against_the_loop<Kmer32bit>(reads, k, 11, 0, FHash::canon_invhash);
    check_against_the_loop<Kmer32bit>(reads, k, 11, 5, FHash::canon_invhash);
    check_against_the_loop<Kmer32bit>(reads, k, 1, 0, FHash::value_masked); // four values of g: ties everywhere, the widest reach
    check_against_the_loop<Kmer32bit>(reads, k, 1, 7, FHash::canon_value);
    check_against_the_loop<Kmer64bit>(reads, k, k, 0, FHash::canon_invhash); // s == k: every k-mer
    // one base repeated and a repeat of period 2, longer than a tile: every k-mer, and ties
    reads = {std::string(1500, 'A'), random_read(state, 300), std::string()};
    for (size_t i = 0; i < 2600; i++) reads[2] += "AC"[i & 1];
    check_against_the_loop<Kmer32bit>(reads, k, 11, 2, FHash::canon_value);
    std::vector<Sequence> poly_a{Sequence(std::string_view(reads[0]))};
    const Minimizers all = read_syncmers<Kmer64bit>(detail::pointers(poly_a), k, 11, 3); // (the overload for sequence pointers)
    CHECK(all.size() == 1500 - k + 1);
    bool refused = false;
    try {
        std::vector<Sequence> one{Sequence(std::string_view(reads[1]))};
        (void) read_syncmers<Kmer64bit>(detail::gather(detail::pointers(one)), k, 11, 6); // t above (k - s) / 2
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
}

}  // namespace

int main() {
    try {
        test_read_syncmers();
        std::printf("ok test_read_syncmers\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_read_syncmers: %s\n", e.what());
        return 1;
    }
}

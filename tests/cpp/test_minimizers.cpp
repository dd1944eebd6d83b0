// test_minimizers -- read_minimizers of the C++ mirror (include/kmerutils.hpp) against the rule written out as a plain loop over
// the mirror's own kmer_hashes: per window of w consecutive k-mers the position of smallest hash, ties to the smallest position,
// each chosen position once.  Three reads.  Without a device it stops with the library's error ("no CPU fallback"): nothing is
// computed on the host.
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

void check_against_the_loop(const std::vector<std::string> &reads, size_t k, uint32_t w, FHash fhash) {
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    const detail::Batch b = detail::gather(detail::pointers(seqs));
    const std::vector<uint64_t> h = kmer_hashes<Kmer64bit>(b, k, fhash);
    const std::vector<uint64_t> h_fwd = kmer_hashes<Kmer64bit>(b, k, FHash::value_masked);
    const std::vector<uint64_t> h_can = kmer_hashes<Kmer64bit>(b, k, FHash::canon_value);
    const std::vector<uint64_t> win = minimizer_layout(b, k, w);
    const Minimizers m = read_minimizers<Kmer64bit>(b, k, w, fhash);
    const bool canonical = fhash == FHash::canon_invhash || fhash == FHash::canon_value || fhash == FHash::canon_raw;
    CHECK(m.offsets.size() == reads.size() + 1 && m.offsets[0] == 0 && m.offsets.back() == m.size());
    CHECK(m.pos.size() == m.size() && m.read.size() == m.size() && m.strand.size() == m.size());
    for (size_t i = 0; i < reads.size(); i++) {
        const uint64_t L = reads[i].size(), nk = L >= k ? L - k + 1 : 0;
        const uint64_t nwin = nk == 0 ? 0 : (nk > w ? nk - w + 1 : 1);
        CHECK(win[i + 1] - win[i] == nwin);
        uint64_t e = m.offsets[i], last = UINT64_MAX;
        for (uint64_t j = 0; j < nwin; j++) {
            uint64_t best = j;
            for (uint64_t p = j; p < std::min<uint64_t>(j + w, nk); p++)
                if (h[b.offsets[i] + p] < h[b.offsets[i] + best]) best = p; // strictly smaller: ties stay with the smallest position
            if (best == last) continue;
            last = best;
            CHECK(e < m.offsets[i + 1]);
            CHECK(m.pos[e] == best && m.read[e] == i && m.hashes[e] == h[b.offsets[i] + best]);
            CHECK(m.strand[e] == (canonical && h_can[b.offsets[i] + best] != h_fwd[b.offsets[i] + best] ? 1 : 0));
            e++;
        }
        CHECK(e == m.offsets[i + 1]);
    }
}

void test_read_minimizers() {
    uint64_t state = 0x5EED;
    // more than two tiles of windows; shorter than k; one window (k <= L < k + w)
    std::vector<std::string> reads = {random_read(state, 2 * KMU_MINIMIZER_TILE + 777), random_read(state, 17), random_read(state, 25)};
    check_against_the_loop(reads, 21, 10, FHash::canon_invhash);
    check_against_the_loop(reads, 21, 1, FHash::value_masked);
    // ties everywhere: a repeat of period 2 and poly-A, longer than a tile
    reads = {std::string(1500, 'A'), random_read(state, 300), std::string()};
    for (size_t i = 0; i < 2600; i++) reads[2] += "AC"[i & 1];
    check_against_the_loop(reads, 21, 19, FHash::canon_value);
    check_against_the_loop(reads, 21, KMU_MINIMIZER_MAX_W, FHash::value_masked);
    bool refused = false;
    try {
        (void) minimizer_layout(detail::Batch{{}, {0, 10}, {}, KMU_INPUT_ASCII}, 21, 0);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
}

}  // namespace

int main() {
    try {
        test_read_minimizers();
        std::printf("ok test_read_minimizers\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_read_minimizers: %s\n", e.what());
        return 1;
    }
}

// test_anchor_match -- match_read_anchors of the C++ mirror (include/kmerutils.hpp) against a brute force over the slices that
// gen_read_anchors returned: read B is the first half of read A, so their windows at 0, 250 and 500 are identical rows; three
// unrelated reads stand by.  Without a device it stops with the library's error ("no CPU fallback").
#include <cstdio>
#include <set>
#include <sstream>
#include <string>
#include <tuple>

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

// minhash_distance (minhash.rs:134-190) on the hashes of two slices: common, total
std::pair<uint32_t, uint32_t> walk(const std::vector<InvHashCount> &a, const std::vector<InvHashCount> &b) {
    const uint32_t n1 = uint32_t(a.size()), n2 = uint32_t(b.size());
    uint32_t i = 0, j = 0, common = 0, total = 0;
    while (i < n1 && j < n2) {
        if (a[i].hashed < b[j].hashed) i++;
        else if (b[j].hashed < a[i].hashed) j++;
        else { i++; j++; common++; }
        total++;
        if (total >= n1) break;
    }
    if (total < n1) {
        if (i < n1) total += n1 - i;
        if (j < n1) total += n1 - j;
        if (total > n1) total = n1;
    }
    return {common, total};
}

void test_match_read_anchors() {
    const uint32_t window = 500, overlap = 250, nbkmer = 16;
    uint64_t state = 0xB10B;
    const std::string genome = random_read(state, 3000);
    std::vector<std::string> reads = {genome, genome.substr(0, 1500), random_read(state, 1200), random_read(state, 700),
                                      random_read(state, 90)};
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    const AnchorsGeneratorParameters params("reads.fasta", window, nbkmer, 21, overlap);
    const auto anchors = gen_read_anchors<Kmer64bit>(params, 3, detail::pointers(seqs));
    std::vector<const SliceAnchor<Kmer64bit> *> slices;
    for (const auto &ra : anchors)
        for (const auto &s : ra.anchors) slices.push_back(&s);

    for (uint32_t n_keys : {1u, 4u})
        for (uint32_t min_common : {0u, 1u, 3u}) {
            // brute force: (a, h*, b) with h* the smallest key the two slices share
            std::vector<std::tuple<size_t, uint64_t, size_t>> want;
            for (size_t a = 0; a < slices.size(); a++)
                for (size_t b = 0; b < slices.size(); b++) {
                    if (slices[a]->readnum == slices[b]->readnum) continue;
                    std::set<uint64_t> ka;
                    for (size_t t = 0; t < slices[a]->minhash.size() && t < n_keys; t++) ka.insert(slices[a]->minhash[t].hashed);
                    uint64_t hstar = UINT64_MAX;
                    bool hit = false;
                    for (size_t t = 0; t < slices[b]->minhash.size() && t < n_keys; t++)
                        if (ka.count(slices[b]->minhash[t].hashed)) {
                            hstar = std::min(hstar, slices[b]->minhash[t].hashed);
                            hit = true;
                        }
                    if (hit && walk(slices[a]->minhash, slices[b]->minhash).first >= min_common) want.emplace_back(a, hstar, b);
                }
            std::sort(want.begin(), want.end());
            const auto got = match_read_anchors<Kmer64bit>(anchors, params, n_keys, min_common);
            CHECK(!want.empty());
            CHECK(got.size() == want.size());
            for (size_t p = 0; p < want.size(); p++) {
                const auto &a = *slices[std::get<0>(want[p])], &b = *slices[std::get<2>(want[p])];
                const auto d = walk(a.minhash, b.minhash);
                CHECK((got[p] == AnchorMatch{a.readnum, a.slicepos, b.readnum, b.slicepos, d.first, d.second}));
            }
            // the windows of A (read 3) and B (read 4) at 0, 250 and 500 are the same bases
            for (uint32_t pos : {0u, 250u, 500u})
                for (int dir = 0; dir < 2; dir++) {
                    const AnchorMatch m{dir ? 4u : 3u, pos, dir ? 3u : 4u, pos, nbkmer, nbkmer};
                    CHECK(std::find(got.begin(), got.end(), m) != got.end());
                }
        }
}

}  // namespace

int main() {
    try {
        test_match_read_anchors();
        std::printf("ok test_match_read_anchors\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_match_read_anchors: %s\n", e.what());
        return 1;
    }
}

// test_anchor_overlaps -- anchor_overlaps and read_overlaps of the C++ mirror (include/kmerutils.hpp).  anchor_overlaps on window
// pairs written here, with the answers worked out by hand; read_overlaps on reads cut from one genome (one reverse-complemented,
// one unrelated) against a vote over the hits of match_read_anchors written in this program by the rules of include/kmu.h.
// Without a device it stops with the library's error ("no CPU fallback").
#include <algorithm>
#include <cstdio>
#include <map>
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

std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

bool same(const kmu_overlap &o, uint32_t a, uint32_t b, uint32_t strand, int32_t diag, uint32_t score, uint32_t votes, uint32_t lo,
          uint32_t hi) {
    return o.read_a == a && o.read_b == b && o.strand == strand && o.diag == diag && o.score == score && o.votes == votes &&
           o.slice_a_min == lo && o.slice_a_max == hi;
}

// reads of 10 rows each: row = 10 * read + slice
void test_hand_cases() {
    const std::vector<uint64_t> off = {0, 10, 20, 30, 40};
    // read 0 x read 1: (slice 2, slice 1) and (slice 3, slice 0): strand 0 has d = 1 and d = 3, strand 1 d = 3 twice
    const std::vector<uint32_t> pairs = {2, 11, 3, 10};
    auto got = anchor_overlaps(pairs, {}, off, off, 2, 2);
    CHECK(got.size() == 1 && same(got[0], 0, 1, 0, 1, 2, 2, 2, 3)); // band 2: a tie at 2, strand 0 first
    got = anchor_overlaps(pairs, {}, off, off, 2, 1);
    CHECK(got.size() == 1 && same(got[0], 0, 1, 1, 3, 2, 2, 2, 3));
    // a band stops at the read pair; weights; min_score; a negative diagonal; upper
    const std::vector<uint32_t> p2 = {5, 10, 7, 21, 8, 20, 10, 37, 11, 39, 37, 10};
    const std::vector<uint32_t> d2 = {1, 9, 9, 10, 9, 9, 3, 9, 9, 1, 9, 9, 1, 9, 9, 7, 9, 9};
    got = anchor_overlaps(p2, d2, off, off, 1, 1);
    CHECK(got.size() == 4);
    CHECK(same(got[0], 0, 1, 0, 5, 1, 1, 5, 5) && same(got[1], 0, 2, 0, 6, 10, 1, 7, 7));
    CHECK(same(got[2], 1, 3, 0, -8, 2, 2, 0, 1) && same(got[3], 3, 1, 0, 7, 7, 1, 7, 7));
    got = anchor_overlaps(p2, d2, off, off, 1, 2, 2, true);
    CHECK(got.size() == 2 && same(got[0], 0, 2, 0, 6, 13, 2, 7, 8) && same(got[1], 1, 3, 0, -8, 2, 2, 0, 1));
    CHECK(anchor_overlaps({}, {}, off, off).empty());
}

void test_read_overlaps() {
    const uint32_t window = 200, overlap = 100, nbkmer = 16, stride = window - overlap;
    uint64_t state = 0x0E11;
    const std::string genome = random_read(state, 4000);
    const std::vector<std::string> reads = {genome.substr(0, 1600),    genome.substr(300, 1600),          genome.substr(1000, 1600),
                                            revcomp(genome.substr(600, 1400)), genome.substr(2200, 1600), random_read(state, 900)};
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    const AnchorsGeneratorParameters params("reads.fasta", window, nbkmer, 21, overlap);
    const uint32_t first = 7;
    const auto anchors = gen_read_anchors<Kmer64bit>(params, first, detail::pointers(seqs), FHash::canon_value);

    for (uint32_t strands : {1u, 2u})
        for (uint32_t band : {0u, 1u, 3u})
            for (uint32_t min_score : {0u, 8u}) {
                // the vote, over the hits of match_read_anchors: (read a, read b) -> (strand, diag) -> weight, votes, first, last
                struct Run {
                    uint64_t w = 0;
                    uint32_t v = 0, lo = UINT32_MAX, hi = 0;
                };
                std::map<std::pair<uint32_t, uint32_t>, std::map<std::pair<uint32_t, int64_t>, Run>> vote;
                for (const AnchorMatch &m : match_read_anchors<Kmer64bit>(anchors, params, 2, 1)) {
                    if (!(m.readnum_a < m.readnum_b)) continue;
                    const int64_t sa = m.slicepos_a / stride, sb = m.slicepos_b / stride;
                    for (uint32_t s = 0; s < strands; s++) {
                        Run &r = vote[{m.readnum_a, m.readnum_b}][{s, s ? sa + sb : sa - sb}];
                        r.w += m.common;
                        r.v++;
                        r.lo = std::min(r.lo, m.slicepos_a);
                        r.hi = std::max(r.hi, m.slicepos_a);
                    }
                }
                std::vector<Overlap> want;
                for (const auto &rp : vote) {
                    bool have = false;
                    uint64_t best = 0;
                    Overlap o{};
                    for (const auto &run : rp.second) { // strand 0 first, then ascending d: the first of the largest wins
                        Run sum;
                        for (int64_t e = run.first.second; e <= run.first.second + int64_t(band); e++) {
                            const auto it = rp.second.find({run.first.first, e});
                            if (it == rp.second.end()) continue;
                            sum.w += it->second.w;
                            sum.v += it->second.v;
                            sum.lo = std::min(sum.lo, it->second.lo);
                            sum.hi = std::max(sum.hi, it->second.hi);
                        }
                        if (!have || sum.w > best) {
                            have = true;
                            best = sum.w;
                            o = Overlap{rp.first.first, rp.first.second, run.first.first, run.first.second * int64_t(stride),
                                        uint32_t(sum.w), sum.v, sum.lo, sum.hi};
                        }
                    }
                    if (best >= min_score) want.push_back(o);
                }
                const auto got = read_overlaps<Kmer64bit>(anchors, params, 2, 1, strands, band, min_score);
                CHECK(!want.empty());
                CHECK(got.size() == want.size());
                for (size_t i = 0; i < want.size(); i++) CHECK(got[i] == want[i]);
                if (strands == 2 && band == 1 && min_score == 8) {
                    auto find = [&](uint32_t a, uint32_t b) {
                        for (const Overlap &o : got)
                            if (o.readnum_a == first + a && o.readnum_b == first + b) return o;
                        throw Failure("a read pair is missing");
                    };
                    // reads 0 and 1 start 300 bases apart on the same strand; read 3 is the reverse complement of genome[600:2000)
                    CHECK(find(0, 1).strand == 0 && std::llabs(find(0, 1).offset - 300) <= 100);
                    CHECK(find(0, 3).strand == 1 && find(1, 3).strand == 1 && find(2, 3).strand == 1);
                    CHECK(std::llabs(find(0, 3).offset - 1800) <= 100);
                    for (const Overlap &o : got) CHECK(o.readnum_b != first + 5);
                }
            }
}

}  // namespace

int main() {
    try {
        test_hand_cases();
        test_read_overlaps();
        std::printf("ok test_anchor_overlaps\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_anchor_overlaps: %s\n", e.what());
        return 1;
    }
}

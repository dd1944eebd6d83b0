// test_chains -- seed_chains / chain_hits / read_chains of the C++ mirror (include/kmerutils.hpp).  A hand-made case whose records
// are known (the same chain on both strands: strand 0 wins), then two reads cut from one sequence, once on the same strand and once
// with the second reverse-complemented: the program prints the reads and the records, and tests/test_cpp_chains.py compares them
// with the Python route on the same reads.  Without a device it stops with the library's error ("no CPU fallback").
#include <algorithm>
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

std::string revcomp(const std::string &s) {
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

void print(const char *what, const std::vector<kmu_chain> &recs) {
    for (const kmu_chain &r : recs)
        std::printf("%s %u %u %u %u %u %u %u %u %u %u\n", what, r.read_a, r.read_b, r.strand, r.score, r.n_seeds, r.n_anchors, r.a_start,
                    r.a_end, r.b_start, r.b_end);
}

void test_by_hand() {
    // read 0 against read 1: (10, 10) -> (30, 30) on the same strand, (10, 60) -> (30, 40) on the opposite one
    Minimizers q, db;
    q.pos = {10, 30, 10, 30};
    q.read = {0, 0, 0, 0};
    q.strand = {0, 0, 0, 0};
    q.offsets = {0, 0, 0};
    db.pos = {10, 30, 60, 40};
    db.read = {1, 1, 1, 1};
    db.strand = {0, 0, 1, 1};
    db.offsets = {0, 0, 0};
    q.hashes.assign(4, 0);
    db.hashes.assign(4, 0);
    kmu_chain_params p{};
    p.span = 15;
    p.max_gap = 100;
    p.band = 100;
    p.min_seeds = 1;
    const std::vector<uint32_t> pairs = {3, 3, 0, 0, 2, 2, 1, 1};
    std::vector<kmu_chain> r = seed_chains(pairs, q, db, p);
    CHECK(r.size() == 1);
    CHECK(r[0].read_a == 0 && r[0].read_b == 1 && r[0].strand == 0 && r[0].score == 30 && r[0].n_seeds == 2 && r[0].n_anchors == 2);
    CHECK(r[0].a_start == 10 && r[0].a_end == 45 && r[0].b_start == 10 && r[0].b_end == 45);
    r = seed_chains({3, 3, 2, 2}, q, db, p);
    CHECK(r.size() == 1 && r[0].strand == 1 && r[0].b_start == 40 && r[0].b_end == 75 && r[0].a_start == 10 && r[0].a_end == 45);
    p.min_seeds = 3;
    CHECK(seed_chains(pairs, q, db, p).empty());
    CHECK(seed_chains({}, q, db, p).empty());
    bool refused = false;
    p.span = 65;
    try {
        (void) seed_chains(pairs, q, db, p);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
}

void test_two_reads(bool opposite) {
    uint64_t state = opposite ? 0xB0B : 0xA11CE;
    const std::string genome = random_read(state, 3000);
    const std::string a = genome.substr(0, 2000), b = genome.substr(1000, 2000);
    const std::vector<std::string> reads = {a, opposite ? revcomp(b) : b, random_read(state, 700)};
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) {
        std::printf("read %s\n", r.c_str());
        seqs.emplace_back(std::string_view(r));
    }
    const detail::Batch batch = detail::gather(detail::pointers(seqs));
    const std::vector<kmu_chain> r = read_chains<Kmer64bit>(batch, 15, 10);
    print("chain", r);
    CHECK(r.size() == 1 && r[0].read_a == 0 && r[0].read_b == 1 && r[0].strand == (opposite ? 1u : 0u));
    CHECK(r[0].a_start >= 1000 && r[0].a_start < 1010 && r[0].a_end > 1990 && r[0].a_end <= 2000);
    // the same through the steps, against a database of its own: both directions of the pair, no filter
    const Minimizers m = read_minimizers<Kmer64bit>(batch, 15, 10);
    const std::vector<kmu_chain> both = chain_hits(m, &m, 15, 0, 5000, 500, 1, 0);
    print("both", both);
    CHECK(std::count_if(both.begin(), both.end(), [](const kmu_chain &c) { return c.read_a != c.read_b && c.n_seeds >= 3; }) == 2);
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_two_reads(false);
        test_two_reads(true);
        std::printf("ok test_chains\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_chains: %s\n", e.what());
        return 1;
    }
}

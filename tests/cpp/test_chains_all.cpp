// test_chains_all -- seed_chains_all / chain_rank / chain_mapq / chain_hits(all) / paf_line with a rank record of the C++ mirror
// (include/kmerutils.hpp).  A hand-made case whose records are known (a main chain, a branch off its first anchor and a chain on the
// other strand), then a contig and a read made of two far-apart pieces of it: the program prints the sequences, the records, the
// ranks and the mapping qualities, and tests/test_cpp_chains_all.py compares them with the Python route on the same sequences.
// Without a device it stops with the library's error ("no CPU fallback").
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

bool same(const kmu_chain &r, uint32_t strand, uint32_t score, uint32_t n_seeds, uint32_t n_anchors, uint32_t a_start, uint32_t a_end,
          uint32_t b_start, uint32_t b_end) {
    return r.read_a == 0 && r.read_b == 1 && r.strand == strand && r.score == score && r.n_seeds == n_seeds && r.n_anchors == n_anchors &&
           r.a_start == a_start && r.a_end == a_end && r.b_start == b_start && r.b_end == b_end;
}

void print(const std::vector<kmu_chain> &recs, const std::vector<kmu_chain_rank_rec> &rank) {
    for (size_t c = 0; c < recs.size(); c++) {
        const kmu_chain &r = recs[c];
        std::printf("all %u %u %u %u %u %u %u %u %u %u\n", r.read_a, r.read_b, r.strand, r.score, r.n_seeds, r.n_anchors, r.a_start, r.a_end,
                    r.b_start, r.b_end);
        std::printf("rank %u %u %u %u\n", rank[c].rank, rank[c].parent, rank[c].sub_score, rank[c].n_sub);
        std::printf("mapq %u\n", chain_mapq(r, rank[c], c));
    }
}

void test_by_hand() {
    // read 0 against read 1: (10, 10) -> (30, 30) -> (50, 50) with a branch (10, 10) -> (30, 34) on the same strand,
    // (10, 60) -> (30, 40) on the opposite one
    Minimizers q, db;
    q.pos = {10, 30, 30, 50, 10, 30};
    q.read = {0, 0, 0, 0, 0, 0};
    q.strand = {0, 0, 0, 0, 0, 0};
    q.offsets = {0, 0, 0};
    db.pos = {10, 30, 34, 50, 60, 40};
    db.read = {1, 1, 1, 1, 1, 1};
    db.strand = {0, 0, 0, 0, 1, 1};
    db.offsets = {0, 0, 0};
    q.hashes.assign(6, 0);
    db.hashes.assign(6, 0);
    kmu_chain_params p{};
    p.span = 15;
    p.max_gap = 100;
    p.band = 100;
    p.min_seeds = 1;
    const std::vector<uint32_t> pairs = {5, 5, 3, 3, 0, 0, 2, 2, 4, 4, 1, 1};
    CHECK(seed_chains(pairs, q, db, p).size() == 1);
    std::vector<kmu_chain> r = seed_chains_all(pairs, q, db, p);
    CHECK(r.size() == 3);
    CHECK(same(r[0], 0, 14, 1, 4, 30, 45, 34, 49) && same(r[1], 0, 45, 3, 4, 10, 65, 10, 65) && same(r[2], 1, 30, 2, 2, 10, 45, 40, 75));
    // all three overlap on the query read: the best one is primary, the others are its secondaries
    const std::vector<kmu_chain_rank_rec> rank = chain_rank(r, 2);
    CHECK(rank.size() == 3 && rank[0].rank == 2 && rank[1].rank == 0 && rank[2].rank == 1);
    CHECK(rank[0].parent == 1 && rank[2].parent == 1 && rank[1].parent == 1 && rank[1].sub_score == 30 && rank[1].n_sub == 2);
    CHECK(rank[0].n_sub == 0 && rank[0].sub_score == 0 && rank[2].n_sub == 0);
    // 40 * (1 - 30 / 45) * min(1, 3 / 10) * ln(45) = 15.2
    CHECK(chain_mapq(r[1], rank[1], 1) == 15 && chain_mapq(r[0], rank[0], 0) == 0 && chain_mapq(r[2], rank[2], 2) == 0);
    const std::vector<kmu_chain_rank_rec> apart = chain_rank(r, 2, 1000);  // only containment masks: the branch lies inside the main chain
    CHECK(apart[0].parent == 1 && apart[2].parent == 1 && apart[1].n_sub == 2);
    kmu_chain_aln a{};
    a.edit = 2;
    a.matches = 50;
    a.flags = KMU_ALN_DONE;
    CHECK(paf_line(r[1], a, "q", 100, "t", 200) == "q\t100\t10\t65\t+\tt\t200\t10\t65\t50\t52\t255\tNM:i:2\ts1:i:45\tcm:i:3");
    CHECK(paf_line(r[1], a, rank[1], 1, "q", 100, "t", 200) == "q\t100\t10\t65\t+\tt\t200\t10\t65\t50\t52\t15\tNM:i:2\ts1:i:45\tcm:i:3\ttp:A:P\ts2:i:30");
    CHECK(paf_line(r[2], a, rank[2], 2, "q", 100, "t", 200) == "q\t100\t10\t45\t-\tt\t200\t40\t75\t50\t52\t0\tNM:i:2\ts1:i:30\tcm:i:2\ttp:A:S\ts2:i:0");
    p.min_seeds = 2;
    r = seed_chains_all(pairs, q, db, p);
    CHECK(r.size() == 2 && same(r[0], 0, 45, 3, 4, 10, 65, 10, 65) && same(r[1], 1, 30, 2, 2, 10, 45, 40, 75));
    CHECK(seed_chains_all({}, q, db, p).empty() && chain_rank({}, 2).empty());
    bool refused = false;
    try {
        (void) chain_rank(r, 2, 1001);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    refused = false;
    std::swap(r[0].read_a, r[1].read_b);  // read_a 1, then 0
    try {
        (void) chain_rank(r, 2);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

void test_chimeric_read() {
    uint64_t state = 0xC41;
    const std::string contig = random_read(state, 6000);
    const std::string read = contig.substr(4000, 1000) + contig.substr(500, 1000);
    std::printf("read %s\ncontig %s\n", read.c_str(), contig.c_str());
    const std::vector<Sequence> reads = {Sequence(std::string_view(read))}, contigs = {Sequence(std::string_view(contig))};
    const detail::Batch bq = detail::gather(detail::pointers(reads)), bdb = detail::gather(detail::pointers(contigs));
    const Minimizers q = read_minimizers<Kmer64bit>(bq, 15, 10), db = read_minimizers<Kmer64bit>(bdb, 15, 10);
    const std::vector<kmu_chain> one = chain_hits(q, &db, 15), every = chain_hits(q, &db, 15, 0, 5000, 500, 3, 0, Context::global(), true);
    CHECK(one.size() == 1 && every.size() == 2);
    const std::vector<kmu_chain_rank_rec> rank = chain_rank(every, 1);
    CHECK(rank[0].parent == 0 && rank[1].parent == 1 && rank[0].n_sub == 0 && rank[1].n_sub == 0);
    print(every, rank);
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_chimeric_read();
        std::printf("ok test_chains_all\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_chains_all: %s\n", e.what());
        return 1;
    }
}

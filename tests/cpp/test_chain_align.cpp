// test_chain_align -- chain_align / align_chains / read_alignments / paf_line of the C++ mirror (include/kmerutils.hpp).  Hand-made
// chains whose records are known, then two reads cut from one sequence with a few edits planted in the second, once on the same
// strand and once with the second reverse-complemented: the program prints the reads, the records and the PAF lines, and
// tests/test_cpp_chain_align.py compares them with the Python route on the same reads.  Without a device it stops with the
// library's error ("no CPU fallback").
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

detail::Batch batch_of(const std::vector<std::string> &reads, std::vector<Sequence> &seqs) {
    seqs.clear();
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    return detail::gather(detail::pointers(seqs));
}

kmu_chain chain(uint32_t ra, uint32_t rb, uint32_t strand, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    kmu_chain c{};
    c.read_a = ra;
    c.read_b = rb;
    c.strand = strand;
    c.score = 30;
    c.n_seeds = 2;
    c.n_anchors = 2;
    c.a_start = a0;
    c.a_end = a1;
    c.b_start = b0;
    c.b_end = b1;
    return c;
}

void test_by_hand() {
    std::vector<Sequence> seqs;
    const std::vector<std::string> reads = {"ACGTACGGTT", "ACGTCAGGTT", revcomp("ACGTACGGTT"), "AAAAAAAA"};
    const detail::Batch b = batch_of(reads, seqs);
    const std::vector<kmu_chain> chains = {chain(0, 1, 0, 0, 10, 0, 10), chain(0, 2, 1, 0, 10, 0, 10), chain(3, 3, 0, 0, 5, 0, 8),
                                           chain(0, 1, 0, 4, 4, 2, 2)};
    std::vector<kmu_chain_aln> r = chain_align(chains, b, nullptr, 2);
    CHECK(r.size() == 4);
    CHECK(r[0].edit == 2 && r[0].matches == 9 && r[0].n_diags == 5 && r[0].flags == (KMU_ALN_DONE | KMU_ALN_EXACT));
    CHECK(r[1].edit == 0 && r[1].matches == 10 && r[1].flags == (KMU_ALN_DONE | KMU_ALN_EXACT));
    CHECK(r[2].edit == 3 && r[2].matches == 5 && r[2].n_diags == 8);
    CHECK(r[3].edit == 0 && r[3].matches == 0 && r[3].n_diags == 5);
    // a database of its own
    std::vector<Sequence> seqs_db;
    const detail::Batch db = batch_of({"ACGTCAGGTT"}, seqs_db);
    r = align_chains({chain(0, 0, 0, 0, 10, 0, 10)}, b, &db, 2);
    CHECK(r.size() == 1 && r[0].edit == 2 && r[0].matches == 9);
    CHECK(chain_align({}, b).empty());
    CHECK(paf_line(chains[0], r[0], "q", 10, "t", 12) == "q\t10\t0\t10\t+\tt\t12\t0\t10\t9\t11\t255\tNM:i:2\ts1:i:30\tcm:i:2");
    kmu_chain_aln skipped{0xFFFFFFFFu, 0, 1289, 0};
    CHECK(paf_line(chain(0, 1, 1, 0, 40, 0, 1200), skipped, "q", 50, "t", 1300) == "q\t50\t0\t40\t-\tt\t1300\t0\t1200\t0\t1200\t255\ts1:i:30\tcm:i:2");
    bool refused = false;
    try {
        (void) chain_align(chains, b, nullptr, KMU_ALIGN_MAX_DIAGS / 2);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    refused = false;
    try {
        (void) chain_align({chain(0, 4, 0, 0, 1, 0, 1)}, b, nullptr, 2);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

void test_two_reads(bool opposite) {
    uint64_t state = opposite ? 0xB0B : 0xA11CE;
    const std::string genome = random_read(state, 3000);
    const std::string a = genome.substr(0, 2000);
    std::string b = genome.substr(1000, 2000);
    for (size_t at = 60; at < 1000; at += 97) b[at] = b[at] == 'A' ? 'C' : 'A'; // substitutions inside the shared part
    b.erase(333, 1);
    b.insert(700, "GG");
    const std::vector<std::string> reads = {a, opposite ? revcomp(b) : b, random_read(state, 700)};
    for (const std::string &r : reads) std::printf("read %s\n", r.c_str());
    std::vector<Sequence> seqs;
    const detail::Batch batch = batch_of(reads, seqs);
    const auto [chains, aln] = read_alignments<Kmer64bit>(batch, 15, 10, FHash::canon_invhash, 0, 5000, 500, 3, 0, 32);
    CHECK(chains.size() == 1 && aln.size() == 1 && chains[0].strand == (opposite ? 1u : 0u));
    CHECK(aln[0].flags == (KMU_ALN_DONE | KMU_ALN_EXACT) && aln[0].edit > 0 && aln[0].edit <= 13);
    const char *names[3] = {"a", "b", "c"};
    for (size_t i = 0; i < chains.size(); i++) {
        const kmu_chain &c = chains[i];
        std::printf("aln %u %u %u %u\n", aln[i].edit, aln[i].matches, aln[i].n_diags, aln[i].flags);
        std::printf("paf %s\n", paf_line(c, aln[i], names[c.read_a], reads[c.read_a].size(), names[c.read_b], reads[c.read_b].size()).c_str());
    }
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_two_reads(false);
        test_two_reads(true);
        std::printf("ok test_chain_align\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_chain_align: %s\n", e.what());
        return 1;
    }
}

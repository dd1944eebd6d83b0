// test_chain_cigar -- chain_cigar / cigar_chains / cigar_string / paf_line with cg:Z: of the C++ mirror (include/kmerutils.hpp).
// Hand-made chains whose paths are known, then a small batch of related reads on both strands: the program prints the reads, the
// chain records, the alignment records, the runs and the PAF lines, and tests/test_cpp_chain_cigar.py compares them with the Python
// route on the same reads.  Without a device it stops with the library's error ("no CPU fallback").
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
    const std::vector<std::string> reads = {"AA", "A", "ACGTACGGTT", "ACGTCAGGTT", revcomp("AC"), "AAC"};
    const detail::Batch b = batch_of(reads, seqs);
    const std::vector<kmu_chain> chains = {chain(0, 1, 0, 0, 2, 0, 1), chain(1, 0, 0, 0, 1, 0, 2), chain(2, 3, 0, 0, 10, 0, 10),
                                           chain(5, 4, 1, 0, 3, 0, 2), chain(2, 3, 0, 4, 4, 2, 2)};
    const ChainCigars r = chain_cigar(chains, b, nullptr, 2);
    CHECK(r.aln.size() == 5 && r.op_offsets.size() == 6 && r.op_offsets[5] == r.ops.size());
    for (const kmu_chain_aln &a : r.aln) CHECK(a.flags == (KMU_ALN_DONE | KMU_ALN_EXACT | KMU_ALN_PATH));
    CHECK(cigar_string(r, 0) == "1I1=" && cigar_string(r, 1) == "1D1=" && cigar_string(r, 2) == "4=1D1=1I4=");
    CHECK(cigar_string(r, 2, false) == "4M1D1M1I4M" && cigar_string(r, 3) == "1I2=" && cigar_string(r, 3, true, true) == "2=1I");
    CHECK(cigar_string(r, 4).empty() && r.aln[4].edit == 0 && r.aln[2].edit == 2 && r.aln[2].matches == 9);
    CHECK(paf_line(chains[3], r, 3, "q", 3, "t", 2) == "q\t3\t0\t3\t-\tt\t2\t0\t2\t2\t3\t255\tNM:i:1\ts1:i:30\tcm:i:2\tcg:Z:2=1I");
    // a budget below every chain's trace: the records of chain_align, no PATH, no runs, and the line without the tag
    const ChainCigars none = cigar_chains(chains, b, nullptr, 2, 255);
    CHECK(none.ops.empty() && none.aln[2].flags == (KMU_ALN_DONE | KMU_ALN_EXACT) && none.aln[2].edit == 2);
    CHECK(paf_line(chains[2], none, 2, "q", 10, "t", 10) == paf_line(chains[2], none.aln[2], "q", 10, "t", 10));
    const ChainCigars empty = chain_cigar({}, b);
    CHECK(empty.aln.empty() && empty.ops.empty() && empty.op_offsets == std::vector<uint64_t>{0});
    bool refused = false;
    try {
        (void) chain_cigar(chains, b, nullptr, KMU_ALIGN_MAX_DIAGS / 2);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    refused = false;
    try {
        (void) chain_cigar({chain(0, 6, 0, 0, 1, 0, 1)}, b, nullptr, 2);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

// six related pairs, every second on the opposite strand, taken whole: printed for the Python route
void test_small_batch() {
    uint64_t state = 0xC16A5;
    std::vector<std::string> reads;
    std::vector<kmu_chain> chains;
    for (uint32_t i = 0; i < 6; i++) {
        const std::string a = random_read(state, 120 + 37 * i);
        std::string b = a;
        for (size_t at = 11; at < b.size(); at += 23 + i) b[at] = b[at] == 'A' ? 'C' : 'A';
        b.erase(40 + i, 1 + i % 3);
        b.insert(90, std::string("GT").substr(0, 1 + i % 2));
        reads.push_back(a);
        reads.push_back(i & 1 ? revcomp(b) : b);
        chains.push_back(chain(2 * i, 2 * i + 1, i & 1, 0, uint32_t(a.size()), 0, uint32_t(b.size())));
    }
    for (const std::string &r : reads) std::printf("read %s\n", r.c_str());
    std::vector<Sequence> seqs;
    const detail::Batch batch = batch_of(reads, seqs);
    const ChainCigars r = cigar_chains(chains, batch, nullptr, 16);
    for (size_t i = 0; i < chains.size(); i++) {
        const kmu_chain &c = chains[i];
        CHECK(r.aln[i].flags == (KMU_ALN_DONE | KMU_ALN_EXACT | KMU_ALN_PATH) && r.aln[i].edit > 0);
        std::printf("chain %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.a_start, c.a_end, c.b_start, c.b_end);
        std::printf("aln %u %u %u %u\n", r.aln[i].edit, r.aln[i].matches, r.aln[i].n_diags, r.aln[i].flags);
        std::printf("ops");
        for (uint64_t x = r.op_offsets[i]; x < r.op_offsets[i + 1]; x++) std::printf(" %u", r.ops[x]);
        std::printf("\n");
        std::printf("paf %s\n", paf_line(c, r, i, "q" + std::to_string(c.read_a), reads[c.read_a].size(), "q" + std::to_string(c.read_b),
                                         reads[c.read_b].size()).c_str());
    }
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_small_batch();
        std::printf("ok test_chain_cigar\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_chain_cigar: %s\n", e.what());
        return 1;
    }
}

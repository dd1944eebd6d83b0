// test_chain_pileup -- chain_pileup / pileup_chains / pile_call of the C++ mirror (include/kmerutils.hpp).  Hand-made chains whose
// votes are known, then a small batch of related reads on both strands: the program prints the reads, the chain records, the rows
// of the shared table and the calls, and tests/test_cpp_chain_pileup.py compares them with the Python route on the same reads.
// Without a device it stops with the library's error ("no CPU fallback").
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

std::vector<uint32_t> row(const std::vector<uint32_t> &table, size_t r) {
    return std::vector<uint32_t>(table.begin() + r * KMU_PILE_COLS, table.begin() + (r + 1) * KMU_PILE_COLS);
}

void test_by_hand() {
    std::vector<Sequence> seqs;
    const std::vector<std::string> reads = {"AA", "A", "AC", "ACG"};  // rows 0-1, 2, 3-4, 5-7
    const detail::Batch b = batch_of(reads, seqs);
    const std::vector<kmu_chain> chains = {chain(0, 1, 0, 0, 2, 0, 1), chain(2, 3, 0, 0, 2, 0, 3)};
    const ChainCigars cg = chain_cigar(chains, b, nullptr, 2);
    CHECK(cigar_string(cg, 0) == "1I1=" && cigar_string(cg, 1) == "2=1D");
    using R = std::vector<uint32_t>;
    const ChainPileups p = chain_pileup(chains, cg, b);
    CHECK(p.shared && p.db.empty() && p.q.size() == 8 * KMU_PILE_COLS && &p.of_db() == &p.q);
    CHECK(row(p.q, 0) == (R{0, 0, 0, 0, 1, 0, 0, 1}) && row(p.q, 1) == (R{1, 0, 0, 0, 0, 0, 0, 1}) && row(p.q, 2) == (R{1, 0, 0, 0, 0, 0, 0, 2}));
    CHECK(row(p.q, 3) == (R{1, 0, 0, 0, 0, 0, 0, 1}) && row(p.q, 4) == (R{0, 1, 0, 0, 0, 1, 1, 1}));
    CHECK(row(p.q, 5) == (R{1, 0, 0, 0, 0, 0, 0, 1}) && row(p.q, 6) == (R{0, 1, 0, 0, 0, 0, 0, 0}) && row(p.q, 7) == (R{0, 0, 0, 0, 1, 0, 0, 1}));
    CHECK(ChainPileups::depth(p.q, 4) == 1 && ChainPileups::depth(p.q, 7) == 1);
    // one side at a time, then both into the tables of the first call: twice the votes
    const ChainPileups a_only = pileup_chains(chains, cg, b, nullptr, KMU_PILE_Q);
    CHECK(!a_only.shared && row(a_only.q, 4) == (R{0, 1, 0, 0, 0, 1, 1, 1}) && row(a_only.q, 5) == (R{0, 0, 0, 0, 0, 0, 0, 0}));
    const ChainPileups b_only = chain_pileup(chains, cg, b, nullptr, KMU_PILE_DB);
    CHECK(row(b_only.q, 7) == (R{0, 0, 0, 0, 1, 0, 0, 1}) && row(b_only.q, 0) == (R{0, 0, 0, 0, 0, 0, 0, 0}));
    const ChainPileups twice = chain_pileup(chains, cg, b, nullptr, KMU_PILE_Q | KMU_PILE_DB, p);
    for (size_t k = 0; k < p.q.size(); k++) CHECK(twice.q[k] == 2 * p.q[k] && p.q[k] == a_only.q[k] + b_only.q[k]);
    // two batches: two tables
    std::vector<Sequence> seqs_db;
    const detail::Batch bdb = batch_of({"A", "ACG"}, seqs_db);
    const std::vector<kmu_chain> across = {chain(0, 0, 0, 0, 2, 0, 1), chain(2, 1, 0, 0, 2, 0, 3)};
    const ChainCigars cg2 = chain_cigar(across, b, &bdb, 2);
    const ChainPileups two = chain_pileup(across, cg2, b, &bdb);
    CHECK(!two.shared && two.q.size() == 8 * KMU_PILE_COLS && two.db.size() == 4 * KMU_PILE_COLS && &two.of_db() == &two.db);
    CHECK(row(two.q, 4) == row(a_only.q, 4) && row(two.db, 3) == row(b_only.q, 7) && row(two.db, 0) == row(b_only.q, 2));
    // calls
    const PileCalls calls = pile_call(p.q, b, 1);
    CHECK(calls.call.size() == 8 && calls.reads.size() == 4);
    CHECK(calls.call[0] == (KMU_PILE_DEL | KMU_CALL_DIFF) && calls.call[1] == KMU_PILE_A && calls.call[4] == (KMU_PILE_C | KMU_CALL_INS));
    CHECK(calls.call[7] == (KMU_PILE_DEL | KMU_CALL_DIFF) && calls.reads[0].n_del == 1 && calls.reads[2].n_ins == 1 && calls.reads[3].depth_sum == 3);
    const PileCalls deep = pile_call(p.q, b, 2);
    for (uint8_t c : deep.call) CHECK(c == KMU_CALL_NONE);
    CHECK(deep.reads[3].covered == 0 && deep.reads[3].max_depth == 1 && deep.reads[3].n_bases == 3);
    const ChainPileups empty = chain_pileup({}, chain_cigar({}, b), b);
    for (uint32_t v : empty.q) CHECK(v == 0);
    bool refused = false;
    try {
        (void) pile_call(p.q, b, 0);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    refused = false;
    ChainCigars wrong = cg;
    wrong.ops[0] = 2u << 4 | KMU_CIGAR_I;  // 2I1= does not sum to m = 2
    try {
        (void) chain_pileup(chains, wrong, b);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

// six related pairs, every second on the opposite strand, taken whole: printed for the Python route
void test_small_batch() {
    uint64_t state = 0xB11E;
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
    for (uint32_t i = 0; i + 1 < 6; i++) chains.push_back(chain(2 * i, 2 * i + 2, 0, 0, 60, 0, 50));  // unrelated reads: many edits
    for (const std::string &r : reads) std::printf("read %s\n", r.c_str());
    std::vector<Sequence> seqs;
    const detail::Batch batch = batch_of(reads, seqs);
    const ChainCigars cg = cigar_chains(chains, batch, nullptr, 16);
    const ChainPileups p = pileup_chains(chains, cg, batch);
    const PileCalls calls = pile_call(p.q, batch, 1);
    for (const kmu_chain &c : chains) std::printf("chain %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.a_start, c.a_end, c.b_start, c.b_end);
    for (size_t r = 0; r * KMU_PILE_COLS < p.q.size(); r++) {
        std::printf("row");
        for (uint32_t k = 0; k < KMU_PILE_COLS; k++) std::printf(" %u", p.q[r * KMU_PILE_COLS + k]);
        std::printf(" call %u\n", calls.call[r]);
    }
    for (const kmu_read_pile &r : calls.reads)
        std::printf("pile %u %u %u %u %u %u %llu\n", r.n_bases, r.covered, r.n_diff, r.n_del, r.n_ins, r.max_depth, (unsigned long long) r.depth_sum);
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_small_batch();
        std::printf("ok test_chain_pileup\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_chain_pileup: %s\n", e.what());
        return 1;
    }
}

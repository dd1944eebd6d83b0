// test_pile_consensus -- pile_ins_plan / chain_pile_ins / pile_consensus / correct_chains of the C++ mirror (include/kmerutils.hpp).
// A hand-made case whose corrected read is known, then a small batch of related reads on both strands: the program prints the
// reads, the chain records, the slot counts, the slot table and the corrected reads, and tests/test_cpp_pile_consensus.py compares
// them with the Python route on the same reads.  Without a device it stops with the library's error ("no CPU fallback").
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

// read 0 is the truth without two of its bases, with one extra base and one wrong base; reads 1 .. 5 are the truth, every second one
// reverse-complemented: the five partners put read 0 right
void test_by_hand() {
    uint64_t state = 0xC0115;
    const std::string truth = random_read(state, 80);
    std::string r0 = truth;
    r0[60] = r0[60] == 'A' ? 'C' : 'A';
    r0.insert(45, 1, truth[45] == 'G' ? 'T' : 'G');
    r0.erase(20, 2);
    std::vector<std::string> reads = {r0};
    std::vector<kmu_chain> chains;
    for (uint32_t r = 1; r <= 5; r++) {
        reads.push_back(r & 1 ? truth : revcomp(truth));
        chains.push_back(chain(0, r, r & 1 ? 0 : 1, 0, uint32_t(r0.size()), 0, 80));
    }
    std::vector<Sequence> seqs;
    const detail::Batch b = batch_of(reads, seqs);
    const ChainCigars cg = chain_cigar(chains, b, nullptr, 8);
    const ChainPileups pile = chain_pileup(chains, cg, b);
    const PileCalls calls = pile_call(pile.q, b, 3);
    const InsPlan plan = pile_ins_plan(pile.q, calls.call, 16);
    CHECK(plan.ins_len.size() == r0.size() + 5 * 80 && plan.n_slots >= 2);
    uint64_t sum = 0, rows = 0;
    for (uint8_t n : plan.ins_len) sum += n, rows += n != 0;
    CHECK(sum == plan.n_slots && rows == 1 && calls.reads[0].n_ins == 1 && calls.reads[0].n_del == 1);
    const ChainInsertions ins = chain_pile_ins(chains, cg, b, plan);
    CHECK(ins.shared && ins.db.empty() && ins.q.size() == plan.n_slots * KMU_INS_COLS && &ins.of_db() == &ins.q);
    uint64_t votes = 0;
    for (uint32_t v : ins.q) votes += v;
    CHECK(votes == 10);  // two letters from each of five partners
    const ConsensusReads cons = pile_consensus(pile.q, calls.call, plan, ins.q, b);
    CHECK(cons.offsets.size() == 7 && cons.read(0) == truth);
    for (uint32_t r = 1; r <= 5; r++) CHECK(cons.read(r) == reads[r]);  // depth 1 is below min_depth: verbatim
    // one side at a time, then both into the table of the first call: twice the votes
    const ChainInsertions a_only = insertions_chains(chains, cg, b, plan, nullptr, nullptr, KMU_PILE_Q);
    const ChainInsertions b_only = chain_pile_ins(chains, cg, b, plan, nullptr, nullptr, KMU_PILE_DB);
    const ChainInsertions twice = chain_pile_ins(chains, cg, b, plan, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, ins);
    for (size_t k = 0; k < ins.q.size(); k++) CHECK(twice.q[k] == 2 * ins.q[k] && ins.q[k] == a_only.q[k] + b_only.q[k]);
    // the whole route in one call
    const CorrectedReads all = correct_chains(chains, b, 8, 3, 16);
    CHECK(all.cons.bases == cons.bases && all.cons.offsets == cons.offsets && all.reads.size() == 6 && all.reads[0].n_ins == 1);
    CHECK(consensus_reads(pile.q, calls.call, plan, ins.q, b).bases == cons.bases);
    // refusals: max_ins out of range; a plan whose sum is not n_slots
    bool refused = false;
    try {
        (void) pile_ins_plan(pile.q, calls.call, 256);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    InsPlan wrong = plan;
    wrong.n_slots += 1;
    std::vector<uint32_t> wide(wrong.n_slots * KMU_INS_COLS, 0u);
    refused = false;
    try {
        (void) pile_consensus(pile.q, calls.call, wrong, wide, b);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    refused = false;
    try {
        (void) chain_pile_ins(chains, cg, b, wrong);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

// eight copies of one sequence with edits of all three kinds, every second on the opposite strand, every pair chained whole:
// printed for the Python route
void test_small_batch() {
    uint64_t state = 0xB11E;
    const std::string root = random_read(state, 300);
    std::vector<std::string> reads;
    for (uint32_t i = 0; i < 8; i++) {
        std::string b = root;
        for (size_t at = 11 + 7 * i; at < b.size(); at += 53 + i) b[at] = b[at] == 'A' ? 'C' : 'A';
        b.erase(40 + 13 * i, 1 + i % 3);
        b.insert(150 + 9 * i, std::string("GTC").substr(0, 1 + i % 3));
        reads.push_back(i & 1 ? revcomp(b) : b);
    }
    std::vector<kmu_chain> chains;
    for (uint32_t i = 0; i < 8; i++)
        for (uint32_t j = i + 1; j < 8; j++) chains.push_back(chain(i, j, (i ^ j) & 1, 0, uint32_t(reads[i].size()), 0, uint32_t(reads[j].size())));
    for (const std::string &r : reads) std::printf("read %s\n", r.c_str());
    for (const kmu_chain &c : chains) std::printf("chain %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.a_start, c.a_end, c.b_start, c.b_end);
    std::vector<Sequence> seqs;
    const detail::Batch batch = batch_of(reads, seqs);
    const ChainCigars cg = cigar_chains(chains, batch, nullptr, 16);
    const ChainPileups p = pileup_chains(chains, cg, batch);
    const PileCalls calls = pile_call(p.q, batch, 3);
    const InsPlan plan = pile_ins_plan(p.q, calls.call, 4);
    const ChainInsertions ins = insertions_chains(chains, cg, batch, plan);
    const ConsensusReads cons = consensus_reads(p.q, calls.call, plan, ins.q, batch);
    std::printf("len");
    for (uint8_t n : plan.ins_len) std::printf(" %u", n);
    std::printf("\n");
    for (size_t s = 0; s < plan.n_slots; s++)
        std::printf("slot %u %u %u %u\n", ins.q[s * 4], ins.q[s * 4 + 1], ins.q[s * 4 + 2], ins.q[s * 4 + 3]);
    for (size_t r = 0; r < reads.size(); r++) std::printf("cons %s\n", cons.read(r).c_str());
    const CorrectedReads all = correct_chains(chains, batch, 16, 3, 4);
    CHECK(all.cons.bases == cons.bases && all.cons.offsets == cons.offsets);
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_small_batch();
        std::printf("ok test_pile_consensus\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_pile_consensus: %s\n", e.what());
        return 1;
    }
}

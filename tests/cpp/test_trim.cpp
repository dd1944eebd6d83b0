// test_trim -- pile_segments / extract_ranges / pile_consensus_pos / trim_reads / correct_trim_chains of the C++ mirror
// (include/kmerutils.hpp).  The hand cases of tests/test_trim_abi.py on tables written out here, then a small batch with a planted
// chimera and a tailed read: the program prints the reads, the chain records, the segments and the trimmed and corrected reads, and
// tests/test_cpp_trim.py compares them with the Python route on the same reads.  Without a device it stops with the library's error
// ("no CPU fallback").
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

detail::Batch batch_of(const std::vector<std::string> &reads, std::vector<Sequence> &seqs) {
    seqs.clear();
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    return detail::gather(detail::pointers(seqs));
}

kmu_chain chain(uint32_t ra, uint32_t rb, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    kmu_chain c{};
    c.read_a = ra;
    c.read_b = rb;
    c.score = 30;
    c.n_seeds = 2;
    c.n_anchors = 2;
    c.a_start = a0;
    c.a_end = a1;
    c.b_start = b0;
    c.b_end = b1;
    return c;
}

// a table whose rows have these depths (all in column A) and these ENDS
std::vector<uint32_t> table(const std::vector<uint32_t> &depths, const std::vector<uint32_t> &ends) {
    std::vector<uint32_t> t(depths.size() * KMU_PILE_COLS, 0u);
    for (size_t g = 0; g < depths.size(); g++) {
        t[g * KMU_PILE_COLS + KMU_PILE_A] = depths[g];
        t[g * KMU_PILE_COLS + KMU_PILE_ENDS] = ends.empty() ? 0u : ends[g];
    }
    return t;
}

bool is_seg(const kmu_pile_seg &s, uint32_t read, uint32_t start, uint32_t end, uint32_t rank) {
    return s.read == read && s.start == start && s.end == end && s.rank == rank;
}

void test_by_hand() {
    // a flush join between rows 2 and 3: whole by depth alone, split by the spanning depth; LONGEST takes the leftmost of equals
    const std::vector<uint32_t> join = table({3, 3, 3, 3, 3, 3}, {3, 0, 3, 3, 0, 3});
    PileSegments s = pile_segments(join, {0, 6}, 3, 0, 1);
    CHECK(s.segs.size() == 1 && is_seg(s.segs[0], 0, 0, 6, 0) && s.reads[0].cls == KMU_TRIM_WHOLE && s.seg_offsets == std::vector<uint64_t>({0, 1}));
    s = pile_segments(join, {0, 6}, 3, 1, 1);
    CHECK(s.segs.size() == 2 && is_seg(s.segs[0], 0, 0, 3, 0) && is_seg(s.segs[1], 0, 3, 6, 1) && s.reads[0].cls == KMU_TRIM_SPLIT);
    CHECK(s.reads[0].n_good == 6 && s.reads[0].kept == 6 && s.reads[0].best_start == 0 && s.reads[0].best_end == 3 && s.reads[0].inner_bad == 0);
    s = pile_segments(join, {0, 6}, 3, 1, 1, true);
    CHECK(s.segs.size() == 1 && is_seg(s.segs[0], 0, 0, 3, 0) && s.reads[0].n_segs == 2);
    s = pile_segments(join, {0, 6}, 3, 1, 4);
    CHECK(s.segs.empty() && s.reads[0].cls == KMU_TRIM_NONE && s.seg_offsets == std::vector<uint64_t>({0, 0}));
    // uncovered ends and a hole, two reads with an empty one between them
    const std::vector<uint32_t> holes = table({0, 3, 3, 3, 1, 0, 4, 4, 2, 5, 5}, {});
    s = pile_segments(holes, {0, 9, 9, 11}, 3, 0, 3);
    CHECK(s.segs.size() == 1 && is_seg(s.segs[0], 0, 1, 4, 0) && s.reads[0].cls == KMU_TRIM_ENDS && s.reads[0].n_good == 5 && s.reads[1].cls == KMU_TRIM_NONE &&
          s.reads[2].cls == KMU_TRIM_NONE && s.reads[2].n_good == 2);
    s = pile_segments(holes, {0, 9, 9, 11}, 3, 0, 2);
    CHECK(s.segs.size() == 3 && is_seg(s.segs[1], 0, 6, 8, 1) && is_seg(s.segs[2], 2, 0, 2, 0) && s.reads[0].inner_bad == 2 && s.reads[2].cls == KMU_TRIM_WHOLE &&
          s.seg_offsets == std::vector<uint64_t>({0, 2, 2, 3}));
    bool refused = false;
    try {
        (void) pile_segments(holes, {0, 9, 9, 11}, 0, 0, 1);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
    // ranges: unordered, empty, overlapping, repeated
    const std::string text = "ACGTacgtNN";
    const std::vector<uint8_t> bytes(text.begin(), text.end());
    const ConsensusReads x = extract_ranges(bytes, {8, 2, 0, 1, 8, 10}, {10, 2, 3, 3, 10, 10});
    CHECK(std::string(x.bases.begin(), x.bases.end()) == "NNACGCGNN" && x.offsets == std::vector<uint64_t>({0, 2, 2, 5, 7, 9, 9}) && x.read(3) == "CG");
    CHECK(extract_ranges(bytes, {}, {}).offsets == std::vector<uint64_t>({0}) && extract_ranges(bytes, {10}, {10}).bases.empty());
    refused = false;
    try {
        (void) extract_ranges(bytes, {0, 5}, {4, 11});
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

// four exact copies of A and of B (120 bases each), a chimera A[:70] + B[70:] and a copy of A with 30 other bases appended; every
// part chained to the matching part of its parents' copies: printed for the Python route
void test_small_batch() {
    uint64_t state = 0x7E1A;
    const std::string a = random_read(state, 120), b = random_read(state, 120);
    std::vector<std::string> reads;
    for (int i = 0; i < 4; i++) reads.push_back(a);
    for (int i = 0; i < 4; i++) reads.push_back(b);
    reads.push_back(a.substr(0, 70) + b.substr(70));
    reads.push_back(a + random_read(state, 30));
    std::vector<kmu_chain> chains;
    for (uint32_t f = 0; f < 8; f += 4)
        for (uint32_t i = f; i < f + 4; i++)
            for (uint32_t j = i + 1; j < f + 4; j++) chains.push_back(chain(i, j, 0, 120, 0, 120));
    for (uint32_t i = 0; i < 4; i++) chains.push_back(chain(8, i, 0, 70, 0, 70));
    for (uint32_t i = 4; i < 8; i++) chains.push_back(chain(8, i, 70, 120, 70, 120));
    for (uint32_t i = 0; i < 4; i++) chains.push_back(chain(9, i, 0, 120, 0, 120));
    for (const std::string &r : reads) std::printf("read %s\n", r.c_str());
    for (const kmu_chain &c : chains) std::printf("chain %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.a_start, c.a_end, c.b_start, c.b_end);
    std::vector<Sequence> seqs;
    const detail::Batch batch = batch_of(reads, seqs);
    const ChainCigars cg = chain_cigar(chains, batch, nullptr, 8);
    const ChainPileups pile = chain_pileup(chains, cg, batch);
    const TrimmedReads t = trim_reads(pile.q, batch, 3, 3, 20);
    CHECK(t.reads.size() == 10 && t.segs.size() == 11 && t.out.offsets.size() == 12);
    CHECK(t.reads[8].cls == KMU_TRIM_SPLIT && is_seg(t.segs[8], 8, 0, 70, 0) && is_seg(t.segs[9], 8, 70, 120, 1));
    CHECK(t.reads[9].cls == KMU_TRIM_ENDS && is_seg(t.segs[10], 9, 0, 120, 0) && t.reads[0].cls == KMU_TRIM_WHOLE);
    CHECK(t.out.read(8) == a.substr(0, 70) && t.out.read(9) == b.substr(70) && t.out.read(10) == a);
    CHECK(trim_reads(pile.q, batch, 3, 0, 20).reads[8].cls == KMU_TRIM_WHOLE);   // depth alone does not see the join
    CHECK(trim_reads(pile.q, batch, 3, 3, 20, true).segs.size() == 10);
    for (const kmu_pile_seg &s : t.segs) std::printf("seg %u %u %u %u\n", s.read, s.start, s.end, s.rank);
    for (size_t r = 0; r + 1 < t.out.offsets.size(); r++) std::printf("trim %s\n", t.out.read(r).c_str());
    // the positions: rows = offsets gives the offsets of the consensus
    const PileCalls calls = pile_call(pile.q, batch, 3);
    const InsPlan plan = pile_ins_plan(pile.q, calls.call, 16);
    const ChainInsertions ins = chain_pile_ins(chains, cg, batch, plan);
    const ConsensusReads cons = pile_consensus(pile.q, calls.call, plan, ins.q, batch);
    const detail::Batch plain = detail::unpacked(batch);
    CHECK(pile_consensus_pos(pile.q, calls.call, plan, ins.q, batch, plain.offsets) == cons.offsets);
    bool refused = false;
    try {
        (void) pile_consensus_pos(pile.q, calls.call, plan, ins.q, batch, {plain.offsets.back() + 1});
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    const CorrectedTrimmedReads all = correct_trim_chains(chains, batch, 8, 3, 16, 3, 20);
    CHECK(all.segs.size() == 11 && all.out.offsets.size() == 12 && all.reads.size() == 10 && all.trims[8].cls == KMU_TRIM_SPLIT);
    CHECK(all.out.read(8) == a.substr(0, 70) && all.out.read(9) == b.substr(70) && all.out.read(10) == a);   // exact copies: nothing to correct
    for (size_t r = 0; r + 1 < all.out.offsets.size(); r++) std::printf("out %s\n", all.out.read(r).c_str());
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_small_batch();
        std::printf("ok test_trim\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_trim: %s\n", e.what());
        return 1;
    }
}

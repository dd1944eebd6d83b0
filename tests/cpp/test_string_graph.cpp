// test_string_graph -- sg_classify / overlap_graph / unitig_labels / gfa_line of the C++ mirror (include/kmerutils.hpp).  The hand
// cases of tests/test_string_graph_abi.py written out here, then planted layout (i): 27 reads of 400 bases every 100 bases of one
// line, with strands and read numbers of the program's own choice.  The program prints the chain records, the arcs and the labels,
// and tests/test_cpp_string_graph.py compares them with the Python route and with the reference on the same records.  Without a
// device it stops with the library's error ("no CPU fallback").
#include <cstdio>
#include <set>
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

kmu_chain chain(uint32_t ra, uint32_t rb, uint32_t s, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
    kmu_chain c{};
    c.read_a = ra;
    c.read_b = rb;
    c.strand = s;
    c.a_start = a0;
    c.a_end = a1;
    c.b_start = b0;
    c.b_end = b1;
    return c;
}

std::vector<uint64_t> offsets_of(const std::vector<uint64_t> &lengths) {
    std::vector<uint64_t> off(1, 0);
    for (uint64_t l : lengths) off.push_back(off.back() + l);
    return off;
}

bool is_arc(const kmu_sg_arc &a, uint32_t from, uint32_t to, uint32_t len, uint32_t ovl, uint32_t rec) {
    return a.from == from && a.to == to && a.len == len && a.ovl == ovl && a.rec == rec && a.zero == 0;
}

GraphParams small() {
    GraphParams g;
    g.min_overlap = 50;
    g.fuzz = 0;
    return g;
}

void test_by_hand() {
    // each of the six classes
    GraphParams g = small();
    g.min_identity_permille = 900;
    std::vector<kmu_chain> chains = {chain(1, 0, 0, 600, 1000, 0, 400), chain(0, 1, 0, 960, 1000, 0, 40),  chain(0, 1, 0, 600, 1000, 0, 400),
                                     chain(0, 1, 0, 300, 700, 300, 700), chain(0, 3, 0, 200, 500, 0, 300), chain(3, 0, 0, 0, 300, 200, 500),
                                     chain(0, 1, 0, 600, 1000, 0, 400)};
    std::vector<kmu_chain_aln> aln(7, kmu_chain_aln{100, 900, 9, KMU_ALN_DONE});
    aln[2] = kmu_chain_aln{0xFFFFFFFFu, 0, 2000, 0};
    const std::vector<uint64_t> off = offsets_of({1000, 1000, 1000, 300});
    const OverlapClasses cls = sg_classify(chains, aln, off, g);
    CHECK((cls.classes == std::vector<uint8_t>{KMU_SG_SKIP, KMU_SG_SHORT, KMU_SG_LOWID, KMU_SG_INTERNAL, KMU_SG_B_CONTAINED, KMU_SG_SKIP, KMU_SG_DOVETAIL}));
    CHECK(cls.reads.size() == 4 && cls.reads[3].flags == KMU_SG_READ_CONTAINED && cls.reads[0].flags == 0 && cls.reads[0].n_records == 5 &&
          cls.reads[1].n_records == 4 && cls.reads[2].n_records == 0 && cls.reads[0].out_fwd == 0);
    const OverlapGraph og = overlap_graph(chains, aln, off, g);
    CHECK(og.classes == cls.classes && og.arcs.size() == 2 && is_arc(og.arcs[0], 0, 2, 600, 400, 6) && is_arc(og.arcs[1], 3, 1, 600, 400, 6));
    CHECK(og.arcs[0].unique == 1 && og.arcs[1].unique == 1 && og.reads[0].out_fwd == 1 && og.reads[1].out_rev == 1 && og.reads[1].out_fwd == 0);
    CHECK((og.arc_offsets == std::vector<uint64_t>{0, 1, 1, 1, 2, 2, 2, 2, 2}));
    // the four strand / side combinations
    const std::vector<kmu_chain> four = {chain(0, 1, 0, 700, 1000, 0, 300), chain(2, 3, 0, 0, 250, 550, 800), chain(4, 5, 1, 700, 1000, 500, 800),
                                         chain(6, 7, 1, 0, 250, 0, 250)};
    const OverlapGraph f = overlap_graph(four, {}, offsets_of({1000, 800, 1000, 800, 1000, 800, 1000, 800}), small());
    CHECK(f.arcs.size() == 8 && is_arc(f.arcs[0], 0, 2, 500, 300, 0) && is_arc(f.arcs[1], 3, 1, 700, 300, 0) && is_arc(f.arcs[2], 5, 7, 550, 250, 1) &&
          is_arc(f.arcs[3], 6, 4, 750, 250, 1) && is_arc(f.arcs[4], 8, 11, 500, 300, 2) && is_arc(f.arcs[5], 10, 9, 700, 300, 2) &&
          is_arc(f.arcs[6], 13, 14, 550, 250, 3) && is_arc(f.arcs[7], 15, 12, 750, 250, 3));
    CHECK(gfa_line(f.arcs[4], "e", "f") == "L\te\t+\tf\t-\t300M" && gfa_line(f.arcs[7], "h", "g") == "L\th\t-\tg\t+\t250M");
    CHECK(gfa_line("e", 1000) == "S\te\t*\tLN:i:1000");
    // no records: no arcs, every summary zero
    const OverlapGraph none = overlap_graph({}, {}, offsets_of({10, 0}), small());
    CHECK(none.arcs.empty() && none.reads.size() == 2 && none.reads[0].n_records == 0 && (none.arc_offsets == std::vector<uint64_t>(5, 0)));
    // a refusal found on the device, and one made before any launch
    bool refused = false;
    try {
        (void) overlap_graph({chain(0, 4, 0, 0, 100, 0, 100)}, {}, off, small());
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    refused = false;
    try {
        g.int_permille = 1001;
        (void) sg_classify(chains, aln, off, g);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
}

void test_tiling() {
    // read i of the line covers [100 i, 100 i + 400); its number is 7 i mod 27 and a generator of the program's own picks its strand
    const uint32_t n = 27;
    uint64_t state = 12;
    std::vector<uint32_t> id(n), flip(n);
    for (uint32_t i = 0; i < n; i++) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        id[i] = (7 * i) % n;
        flip[i] = uint32_t(state >> 40) & 1u;
    }
    std::vector<kmu_chain> chains;
    for (uint32_t d = 1; d <= 3; d++) // every pair that shares at least 50 bases, the pairs of one distance together
        for (uint32_t i = 0; i + d < n; i++) {
            const uint32_t j = i + d, lo = 100 * j, hi = 100 * i + 400; // the shared part of the line
            const uint32_t a = id[i] < id[j] ? i : j, b = a == i ? j : i;
            auto on_read = [&](uint32_t r, uint32_t &s, uint32_t &e) {
                const uint32_t r0 = 100 * r, r1 = r0 + 400;
                s = flip[r] ? r1 - hi : lo - r0;
                e = flip[r] ? r1 - lo : hi - r0;
            };
            uint32_t a0, a1, b0, b1;
            on_read(a, a0, a1);
            on_read(b, b0, b1);
            chains.push_back(chain(id[a], id[b], flip[a] ^ flip[b], a0, a1, b0, b1));
        }
    CHECK(chains.size() == 75);
    for (const kmu_chain &c : chains) std::printf("chain %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.a_start, c.a_end, c.b_start, c.b_end);
    const std::vector<uint64_t> off = offsets_of(std::vector<uint64_t>(n, 400));
    const OverlapGraph g = overlap_graph(chains, {}, off, small());
    std::set<uint32_t> reduced;
    size_t alive = 0, unique = 0;
    for (const kmu_sg_arc &a : g.arcs) {
        if (a.flags & KMU_SG_ARC_REDUCED) reduced.insert(a.rec);
        else alive++;
        unique += a.unique;
        std::printf("arc %u %u %u %u %u %u %u\n", a.from, a.to, a.len, a.ovl, a.rec, a.flags, a.unique);
    }
    CHECK(g.arcs.size() == 150 && reduced.size() == 49 && alive == 52 && unique == 52 && g.arc_offsets.back() == 150);
    for (uint32_t c : reduced) CHECK(c >= 26); // the records of distance 1 come first and survive
    size_t ends = 0;
    for (const kmu_sg_read &r : g.reads) {
        CHECK(r.flags == 0 && r.n_records >= 3 && r.out_fwd <= 1 && r.out_rev <= 1);
        ends += (r.out_fwd == 0) + (r.out_rev == 0);
    }
    CHECK(ends == 2);
    const std::vector<uint32_t> labels = unitig_labels(g.arcs, n);
    CHECK(labels == std::vector<uint32_t>(n, 0));
    std::printf("end\n");
}

}  // namespace

int main() {
    try {
        test_by_hand();
        test_tiling();
        std::printf("ok test_string_graph\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_string_graph: %s\n", e.what());
        return 1;
    }
}

// test_clean -- sg_clean / clean_graph / layout_reads of the C++ mirror (include/kmerutils.hpp).  A hand case written out here; then,
// given a file of arcs (the number of reads, the two limits, one arc per line: from to len ovl rec flags unique), sg_clean,
// clean_graph with three rounds and sg_unitigs over layout_reads on them: the program prints the arcs, the summaries, the counts and
// the unitigs, and tests/test_cpp_clean.py compares them with the arrays of the Python reference.  Without a device it stops with
// the library's error ("no CPU fallback").
#include <algorithm>
#include <cstdio>
#include <fstream>
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

kmu_sg_arc arc(uint32_t from, uint32_t to, uint32_t rec) {
    kmu_sg_arc a{};
    a.from = from;
    a.to = to;
    a.len = 400;
    a.rec = rec;
    return a;
}

void print_stats(const char *word, const kmu_sg_clean_stats &s) {
    std::printf("%s %llu %llu %llu %llu %llu %llu %llu %llu\n", word, (unsigned long long) s.n_tips, (unsigned long long) s.n_tip_reads,
                (unsigned long long) s.n_spared, (unsigned long long) s.n_bubbles, (unsigned long long) s.n_bubble_reads,
                (unsigned long long) s.n_arcs_tip, (unsigned long long) s.n_arcs_bubble, (unsigned long long) s.n_arcs_left);
}

void test_by_hand() {
    // the line 0 -> 1 -> 2 -> 3 -> 4 -> 5 of forward reads and read 6, which enters read 3 beside read 2: arcs with their mates, sorted
    std::vector<kmu_sg_arc> arcs;
    for (uint32_t i = 0; i < 5; i++) {
        arcs.push_back(arc(2 * i, 2 * i + 2, i));
        arcs.push_back(arc(2 * i + 3, 2 * i + 1, i));
    }
    arcs.push_back(arc(12, 6, 5));
    arcs.push_back(arc(7, 13, 5));
    std::sort(arcs.begin(), arcs.end(), [](const kmu_sg_arc &a, const kmu_sg_arc &b) { return a.from != b.from ? a.from < b.from : a.to < b.to; });
    const CleanGraph c = sg_clean(arcs, {}, 7);
    CHECK(c.stats.n_tips == 1 && c.stats.n_tip_reads == 1 && c.stats.n_spared == 1 && c.stats.n_arcs_tip == 2 && c.stats.n_arcs_left == 10);
    CHECK(c.reads.size() == 7 && c.reads[6].flags == KMU_SG_READ_TIP && c.reads[3].flags == 0 && c.reads[3].out_rev == 1);
    for (const kmu_sg_arc &x : c.arcs) CHECK((x.rec == 5) == (x.flags == KMU_SG_ARC_TIP) && x.unique == (x.rec == 5 ? 0u : 1u));
    const std::vector<kmu_sg_read> laid = layout_reads(c.reads);
    CHECK(laid[6].flags == (KMU_SG_READ_TIP | KMU_SG_READ_CONTAINED) && laid[0].flags == 0 && c.reads[6].flags == KMU_SG_READ_TIP);
    const Unitigs u = sg_unitigs(c.arcs, laid, std::vector<uint64_t>{0, 1000, 2000, 3000, 4000, 5000, 6000, 7000});
    CHECK(u.unitigs.size() == 1 && u.unitigs[0].n_reads == 6 && u.unitigs[0].len == 3000 && u.place[6].unitig == KMU_SG_NONE);
    // a second round finds nothing, and clean_graph stops after it
    const CleanGraph again = clean_graph(arcs, {}, 7, 4, 8, 5);
    CHECK(again.stats.n_tips == 1 && again.stats.n_arcs_tip == 2 && again.stats.n_arcs_left == 10 && again.arcs.size() == arcs.size());
    CHECK(clean_graph(arcs, {}, 7, 4, 8, 0).stats.n_arcs_left == 0 && clean_graph(arcs, {}, 7, 4, 8, 0).arcs.size() == arcs.size());
    // with both phases off only unique and the degrees are recomputed
    const CleanGraph off = sg_clean(arcs, {}, 7, 0, 0);
    CHECK(off.stats.n_arcs_left == 12 && off.reads[3].out_rev == 2 && off.reads[6].flags == 0);
    // a refusal found on the device (an arc without its mate), and one made before any launch
    bool refused = false;
    try {
        (void) sg_clean({arc(0, 2, 0)}, {}, 7);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    refused = false;
    try {
        (void) sg_clean(arcs, {}, 7, 65, 8);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused);
}

void test_arcs(const char *path) {
    std::ifstream in(path);
    uint32_t n_reads = 0, T = 0, B = 0;
    CHECK(bool(in >> n_reads >> T >> B));
    std::vector<kmu_sg_arc> arcs;
    kmu_sg_arc a{};
    while (in >> a.from >> a.to >> a.len >> a.ovl >> a.rec >> a.flags >> a.unique) arcs.push_back(a);
    const CleanGraph c = sg_clean(arcs, {}, n_reads, T, B);
    for (const kmu_sg_arc &x : c.arcs) std::printf("arc %u %u %u %u %u %u %u %u\n", x.from, x.to, x.len, x.ovl, x.rec, x.flags, x.unique, x.zero);
    for (const kmu_sg_read &r : c.reads) std::printf("read %u %u %u %u\n", r.flags, r.n_records, r.out_fwd, r.out_rev);
    print_stats("stats", c.stats);
    print_stats("rounds", clean_graph(arcs, {}, n_reads, T, B, 3).stats);
    std::vector<uint64_t> off(size_t(n_reads) + 1, 0); // reads of 1 000 bases: every arc is shorter
    for (size_t r = 0; r <= n_reads; r++) off[r] = 1000u * r;
    const Unitigs u = sg_unitigs(c.arcs, layout_reads(c.reads), off);
    std::printf("unitigs %zu %zu\n", u.unitigs.size(), u.path.size());
    std::printf("end\n");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        test_by_hand();
        if (argc > 1) test_arcs(argv[1]);
        std::printf("ok test_clean\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_clean: %s\n", e.what());
        return 1;
    }
}

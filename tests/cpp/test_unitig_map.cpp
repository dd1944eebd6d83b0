// test_unitig_map -- sg_unitig_chains / unitig_read_chains / polish_unitigs of the C++ mirror (include/kmerutils.hpp).  A hand case
// written out here; then, given a file (the counts and the number of rounds; the unitigs, the steps, the places, the chain records
// with their classes, one record per line; the reads, one per line), the map and polish_unitigs on them: the program prints the
// records, the counts, the polished unitigs and the polished ends, and tests/test_cpp_unitig_map.py compares them with the Python
// reference and the Python route.  Without a device it stops with the library's error ("no CPU fallback").
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

detail::Batch batch_of(const std::vector<std::string> &reads) {
    detail::Batch b;
    b.offsets.assign(1, 0);
    for (const std::string &r : reads) {
        b.bytes.insert(b.bytes.end(), r.begin(), r.end());
        b.offsets.push_back(b.offsets.back() + r.size());
    }
    b.bytes.resize(b.bytes.size() + 16, 0);
    return b;
}

void test_by_hand() {
    // a line of 1 200 bases under three reads of 1 000, each 100 to the right of the one before, and a fourth read, bases 300 .. 700
    // of the line with one base substituted, that lies in read 1
    std::string line(1200, 'A');
    uint64_t x = 88172645463325252ull;
    for (char &c : line) {
        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
        c = "ACGT"[x & 3];
    }
    std::string inner = line.substr(300, 400);
    inner[200] = inner[200] == 'A' ? 'C' : 'A';
    const detail::Batch reads = batch_of({line.substr(0, 1000), line.substr(100, 1000), line.substr(200, 1000), inner});
    Unitigs layout;
    layout.unitigs = {kmu_sg_unitig{0, 1200, 3, 0, 0, 0}};
    layout.path = {kmu_sg_step{0, 0, 1000}, kmu_sg_step{1, 0, 1100}, kmu_sg_step{2, 0, 1200}};
    layout.place = {kmu_sg_place{0, 0, 0, 0}, kmu_sg_place{0, 1, 0, 0}, kmu_sg_place{0, 2, 0, 0}, kmu_sg_place{KMU_SG_NONE, 0, 0, 0}};
    const std::vector<kmu_chain> chains = {kmu_chain{1, 3, 0, 0, 0, 0, 200, 600, 0, 400}};
    const UnitigChains map = unitig_read_chains(layout, chains, {KMU_SG_B_CONTAINED}, reads.offsets);
    CHECK(map.records.size() == 4 && map.stats.n_layout == 3 && map.stats.n_contained == 1 && map.stats.n_unplaced == 0);
    const kmu_chain &c = map.records[3];
    CHECK(c.read_a == 0 && c.read_b == 3 && c.strand == 0 && c.score == 1 && c.n_seeds == 0 && c.n_anchors == 1);
    CHECK(c.a_start == 300 && c.a_end == 700 && c.b_start == 0 && c.b_end == 400);
    CHECK(map.records[1].a_start == 100 && map.records[1].a_end == 1100 && map.records[1].score == 0 && map.records[1].n_seeds == KMU_SG_NONE);
    // without records the contained read stays unplaced
    const UnitigChains bare = sg_unitig_chains(layout, {}, {}, reads.offsets);
    CHECK(bare.records.size() == 3 && bare.stats.n_unplaced == 1);
    const UnitigSequences draft = unitig_sequences(layout, reads.bytes, reads.offsets);
    CHECK(std::string(draft.seq.begin(), draft.seq.end()) == line);
    for (uint32_t rounds = 1; rounds <= 2; rounds++) {
        const PolishedUnitigs p = polish_unitigs(layout, draft, reads, chains, {KMU_SG_B_CONTAINED}, 64, 0, 2, 16, rounds);
        CHECK(p.cons.read(0) == line && p.layout.unitigs[0].len == 1200 && p.layout.path[2].end == 1200 && p.layout.path[0].end == 1000);
        CHECK(p.aln.size() == 4 && p.aln[0].edit == 0 && p.aln[3].edit == 1 && p.summaries.size() == 1 && p.records[3].a_start == 300);
    }
    // a refusal found on the device (a place that names another read's step), and one made before any launch
    bool refused = false;
    try {
        Unitigs bad = layout;
        bad.place[0].rank = 1;
        (void) sg_unitig_chains(bad, chains, {KMU_SG_B_CONTAINED}, reads.offsets);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    refused = false;
    try {
        (void) sg_unitig_chains(layout, chains, {}, reads.offsets);
    } catch (const std::invalid_argument &) {
        refused = true;
    }
    CHECK(refused);
}

void test_file(const char *path) {
    std::ifstream in(path);
    size_t n_unitigs = 0, n_steps = 0, n_reads = 0, n_chains = 0;
    uint32_t rounds = 1;
    CHECK(bool(in >> n_unitigs >> n_steps >> n_reads >> n_chains >> rounds));
    Unitigs layout;
    layout.unitigs.resize(n_unitigs);
    layout.path.resize(n_steps);
    layout.place.resize(n_reads);
    std::vector<kmu_chain> chains(n_chains);
    std::vector<uint8_t> classes(n_chains);
    for (kmu_sg_unitig &u : layout.unitigs) CHECK(bool(in >> u.first >> u.len >> u.n_reads >> u.flags >> u.min_read >> u.zero));
    for (kmu_sg_step &s : layout.path) CHECK(bool(in >> s.read >> s.strand >> s.end));
    for (kmu_sg_place &p : layout.place) CHECK(bool(in >> p.unitig >> p.rank >> p.strand >> p.zero));
    for (size_t i = 0; i < n_chains; i++) {
        kmu_chain &c = chains[i];
        uint32_t cls = 0;
        CHECK(bool(in >> c.read_a >> c.read_b >> c.strand >> c.score >> c.n_seeds >> c.n_anchors >> c.a_start >> c.a_end >> c.b_start >> c.b_end >> cls));
        classes[i] = uint8_t(cls);
    }
    std::vector<std::string> reads(n_reads);
    for (std::string &r : reads) CHECK(bool(in >> r));
    const detail::Batch batch = batch_of(reads);
    const UnitigChains map = sg_unitig_chains(layout, chains, classes, batch.offsets);
    for (const kmu_chain &c : map.records)
        std::printf("rec %u %u %u %u %u %u %u %u %u %u\n", c.read_a, c.read_b, c.strand, c.score, c.n_seeds, c.n_anchors, c.a_start, c.a_end, c.b_start,
                    c.b_end);
    std::printf("stats %llu %llu %llu\n", (unsigned long long) map.stats.n_layout, (unsigned long long) map.stats.n_contained,
                (unsigned long long) map.stats.n_unplaced);
    const PolishedUnitigs p = polish_unitigs(layout, unitig_sequences(layout, batch.bytes, batch.offsets), batch, chains, classes, 64, 0, 2, 16, rounds);
    for (size_t u = 0; u < n_unitigs; u++) std::printf("cons %s\n", p.cons.read(u).c_str());
    for (const kmu_sg_step &s : p.layout.path) std::printf("step %u %u %llu\n", s.read, s.strand, (unsigned long long) s.end);
    for (const kmu_sg_unitig &u : p.layout.unitigs) std::printf("len %llu\n", (unsigned long long) u.len);
    for (const kmu_chain_aln &a : p.aln) std::printf("aln %u %u %u %u\n", a.edit, a.matches, a.n_diags, a.flags);
    for (const kmu_chain &c : p.records) std::printf("used %u %u %u\n", c.read_b, c.a_start, c.a_end);
    std::printf("end\n");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        test_by_hand();
        if (argc > 1) test_file(argv[1]);
        std::printf("ok test_unitig_map\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_unitig_map: %s\n", e.what());
        return 1;
    }
}

// test_unitigs -- sg_unitigs / unitig_sequences / unitig_gfa_line of the C++ mirror (include/kmerutils.hpp).  Hand cases of
// tests/test_unitigs_abi.py written out here; then, given a file of chain records (the number of reads, their lengths, one record
// per line), overlap_graph, sg_unitigs and unitig_sequences on them: the program prints the unitigs and the steps, and
// tests/test_cpp_unitigs.py compares them with the Python route on the same records.  Without a device it stops with the library's
// error ("no CPU fallback").
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

kmu_sg_arc arc(uint32_t from, uint32_t to, uint32_t len, uint32_t unique = 1) {
    kmu_sg_arc a{};
    a.from = from;
    a.to = to;
    a.len = len;
    a.unique = unique;
    return a;
}

std::vector<uint64_t> offsets_of(const std::vector<uint64_t> &lengths) {
    std::vector<uint64_t> off(1, 0);
    for (uint64_t l : lengths) off.push_back(off.back() + l);
    return off;
}

bool is_step(const kmu_sg_step &s, uint32_t read, uint32_t strand, uint64_t end) { return s.read == read && s.strand == strand && s.end == end; }

std::string text(const std::vector<uint8_t> &v) { return std::string(v.begin(), v.end()); }

void test_by_hand() {
    // three reads of 10 bases, each 4 to the right of the one before; read 1 is stored as its reverse complement
    const std::string genome = "ACGTTGCAAGGCTTACGA";
    const std::string r0 = genome.substr(0, 10), r2 = genome.substr(8, 10);
    std::string r1;
    for (size_t i = 0; i < 10; i++) r1 += std::string("TGCA")[std::string("ACGT").find(genome[13 - i])];
    const std::string all = r0 + r1 + r2;
    const std::vector<uint8_t> bases(all.begin(), all.end());
    const std::vector<uint64_t> off = offsets_of({10, 10, 10});
    const std::vector<kmu_sg_arc> arcs = {arc(4, 0, 9, 0), arc(0, 3, 4), arc(2, 1, 4), arc(3, 4, 4), arc(5, 2, 4)};
    const Unitigs u = sg_unitigs(arcs, {}, off);
    CHECK(u.unitigs.size() == 1 && u.unitigs[0].first == 0 && u.unitigs[0].len == 18 && u.unitigs[0].n_reads == 3 && u.unitigs[0].flags == 0 &&
          u.unitigs[0].min_read == 0);
    CHECK(u.path.size() == 3 && is_step(u.path[0], 0, 0, 10) && is_step(u.path[1], 1, 1, 14) && is_step(u.path[2], 2, 0, 18));
    CHECK(u.place.size() == 3 && u.place[1].unitig == 0 && u.place[1].rank == 1 && u.place[1].strand == 1 && u.place[2].rank == 2);
    const UnitigSequences s = unitig_sequences(u, bases, off);
    CHECK(text(s.seq) == genome && (s.seq_offsets == std::vector<uint64_t>{0, 18}));
    CHECK(unitig_gfa_line(0, u.unitigs[0], text(s.seq)) == "S\tutg000000l\t" + genome + "\tLN:i:18");
    CHECK(unitig_gfa_line(0, u.unitigs[0], u.path[1], u.path[0].end, "b") == "a\tutg000000l\t10\tb\t-\t4");
    // a contained read is on no unitig; without arcs every other read is its own
    std::vector<kmu_sg_read> reads(3, kmu_sg_read{});
    reads[1].flags = KMU_SG_READ_CONTAINED;
    const Unitigs alone = sg_unitigs({}, reads, off);
    CHECK(alone.unitigs.size() == 2 && alone.path.size() == 2 && alone.place[1].unitig == KMU_SG_NONE && alone.place[2].unitig == 1 &&
          alone.unitigs[1].min_read == 2 && alone.unitigs[1].first == 1 && alone.unitigs[1].len == 10);
    CHECK(text(unitig_sequences(alone, bases, off).seq) == r0 + r2);
    // a circle of three reads
    const std::vector<kmu_sg_arc> ring = {arc(0, 2, 3), arc(2, 4, 5), arc(4, 0, 7), arc(3, 1, 3), arc(5, 3, 5), arc(1, 5, 7)};
    const Unitigs c = sg_unitigs(ring, {}, off);
    CHECK(c.unitigs.size() == 1 && c.unitigs[0].flags == KMU_SG_UNITIG_CIRCULAR && c.unitigs[0].len == 15 && is_step(c.path[0], 0, 0, 7) &&
          is_step(c.path[1], 1, 0, 10) && is_step(c.path[2], 2, 0, 15));
    CHECK(unitig_gfa_line(7, c.unitigs[0], "x").substr(0, 13) == "S\tutg000007c\t");
    // a refusal found on the device (an arc without its mate), and one made before any launch
    bool refused = false;
    try {
        (void) sg_unitigs({arc(0, 3, 4)}, {}, off);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
    refused = false;
    try {
        Unitigs bad = u;
        bad.path[2].end = 17;
        (void) unitig_sequences(bad, bases, off);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_UNSUPPORTED;
    }
    CHECK(refused);
}

void test_records(const char *path) {
    std::ifstream in(path);
    size_t n = 0;
    CHECK(bool(in >> n));
    std::vector<uint64_t> lengths(n);
    for (auto &l : lengths) CHECK(bool(in >> l));
    std::vector<kmu_chain> chains;
    kmu_chain c{};
    while (in >> c.read_a >> c.read_b >> c.strand >> c.a_start >> c.a_end >> c.b_start >> c.b_end) chains.push_back(c);
    const std::vector<uint64_t> off = offsets_of(lengths);
    GraphParams g;
    g.min_overlap = 50;
    g.fuzz = 0;
    const OverlapGraph graph = overlap_graph(chains, {}, off, g);
    const Unitigs u = sg_unitigs(graph.arcs, graph.reads, off);
    for (const kmu_sg_unitig &x : u.unitigs)
        std::printf("unitig %llu %llu %u %u %u\n", (unsigned long long) x.first, (unsigned long long) x.len, x.n_reads, x.flags, x.min_read);
    for (const kmu_sg_step &s : u.path) std::printf("step %u %u %llu\n", s.read, s.strand, (unsigned long long) s.end);
    for (const kmu_sg_place &p : u.place) std::printf("place %u %u %u\n", p.unitig, p.rank, p.strand);
    const std::vector<uint8_t> bases(off.back(), uint8_t('A'));
    const UnitigSequences s = unitig_sequences(u, bases, off);
    std::printf("bytes %zu\n", s.seq.size());
    std::printf("end\n");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        test_by_hand();
        if (argc > 1) test_records(argv[1]);
        std::printf("ok test_unitigs\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_unitigs: %s\n", e.what());
        return 1;
    }
}

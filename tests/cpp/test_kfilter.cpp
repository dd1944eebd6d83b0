// test_kfilter -- KmerPrefilter / count_repeated_kmers of the C++ mirror (include/kmerutils.hpp).  A hand case written out here;
// then, given a file of reads (first line: k, filter bits per k-mer, hashes; one read per line) and a file of canonical k-mer
// values to ask about, count_repeated_kmers on them: the program prints the number of passing occurrences, the filter's summary,
// its words, the class of every value asked and the entries of the dump, and tests/test_cpp_kfilter.py compares them with the
// numpy model and the oracle.  Without a device it stops with the library's error ("no CPU fallback").
#include <cmath>
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

const char *const READ_A = "ACGTTGCAAGGCTTACGATCGGATCCTTAGGCATGCAAGT";   // 40 bases: 10 31-mers
const char *const READ_B = "TTGACCGGTAAACGTTCAGGCATTTGACCATGGTACCAGA";

void test_by_hand() {
    // (plain host code: no device yet)
    CHECK(kmu_kfilter_cells_for(0, 16) == 1 && kmu_kfilter_cells_for(4, 16) == 1 && kmu_kfilter_cells_for(5, 16) == 2);
    CHECK(kmu_kfilter_cells_for(uint64_t(1) << 40, 16) == 0 && KmerPrefilter<Kmer64bit>::cells_for(1000, 8) == 125);
    const std::vector<Sequence> reads{Sequence(READ_A), Sequence(READ_B), Sequence(READ_A)};
    RepeatedKmers<Kmer64bit> r = count_repeated_kmers<Kmer64bit>(reads, 31, 16);
    const kmu_kfilter_info_t fi = r.filter->info();
    CHECK(fi.n_added == 30 && fi.n_hashes == 4 && fi.kmer_size == 31 && fi.bytes == 16 * fi.n_cells && fi.n_cells == 8);
    CHECK(fi.bits_a >= fi.bits_b && fi.bits_b > 0 && std::isfinite(fi.est_distinct));
    CHECK(r.nb_passed >= 20 && r.nb_passed == r.filter->nb_passing(detail::gather(detail::pointers(reads))));
    const std::vector<Kmer64bit> ka = KmerGenerator<Kmer64bit>(31).generate_kmer(reads[0]), kb = KmerGenerator<Kmer64bit>(31).generate_kmer(reads[1]);
    for (const Kmer64bit &k : ka) {
        const Kmer64bit c = k.reverse_complement().min(k);
        CHECK(r.filter->seen_class(c) == 2 && r.counter->get_count(c) == 2 && r.counter->get_above2_count(c) == 2);
    }
    for (const Kmer64bit &k : kb) {   // seen once: absent, or held with its exact count of 1
        const Kmer64bit c = k.reverse_complement().min(k);
        CHECK(r.filter->seen_class(c) >= 1 && r.counter->get_count(c) == (r.filter->seen_class(c) == 2 ? 1u : 0u));
    }
    CHECK(r.counter->above2_entries().first.size() == 10);
    // two half filters merged are the whole filter; a filter of other parameters is refused
    KmerPrefilter<Kmer64bit> f1(31, 8), f2(31, 8), f3(31, 9);
    f1.insert_reads(detail::pointers(std::vector<Sequence>{reads[0], reads[1]}));
    f2.insert_reads(detail::pointers(std::vector<Sequence>{reads[2]}));
    f1.merge(f2);
    CHECK(f1.words() == r.filter->words() && f1.info().n_added == 30);
    bool refused = false;
    try {
        f1.merge(f3);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG;
    }
    CHECK(refused && f1.words() == r.filter->words());
    // insert_kmer is insert_reads, k-mer by k-mer
    for (const Sequence &s : reads)
        for (const Kmer64bit &k : KmerGenerator<Kmer64bit>(31).generate_kmer(s)) f3.insert_kmer(k.reverse_complement().min(k));
    KmerPrefilter<Kmer64bit> f4(31, 9);
    f4.insert_reads(detail::pointers(reads));
    CHECK(f3.words() == f4.words());
}

template <class Kmer> void run_file(const std::vector<Sequence> &reads, uint8_t k, uint32_t bits, uint32_t hashes, const std::vector<uint64_t> &ask) {
    RepeatedKmers<Kmer> r = count_repeated_kmers<Kmer>(reads, k, 16, bits, hashes);
    const kmu_kfilter_info_t fi = r.filter->info();
    std::printf("passed %llu\n", (unsigned long long) r.nb_passed);
    std::printf("info %llu %llu %llu %llu\n", (unsigned long long) fi.n_cells, (unsigned long long) fi.n_added, (unsigned long long) fi.bits_a,
                (unsigned long long) fi.bits_b);
    for (uint64_t w : r.filter->words()) std::printf("word %llu\n", (unsigned long long) w);
    std::vector<Kmer> kmers;
    for (uint64_t v : ask) kmers.push_back(Kmer::build(typename Kmer::Val(v), k));
    const std::vector<uint8_t> cls = r.filter->seen_class(kmers);
    for (size_t i = 0; i < ask.size(); i++) std::printf("class %llu %u\n", (unsigned long long) ask[i], unsigned(cls[i]));
    const auto [vals, counts] = r.counter->above2_entries();
    for (size_t i = 0; i < vals.size(); i++) std::printf("entry %llu %u\n", (unsigned long long) vals[i], counts[i]);
    std::printf("held %llu %llu\n", (unsigned long long) r.counter->get_nb_distinct(), (unsigned long long) r.counter->get_nb_unique());
    std::printf("end\n");
}

void test_files(const char *reads_path, const char *ask_path) {
    std::ifstream in(reads_path);
    unsigned k = 0, bits = 0, hashes = 0;
    CHECK(bool(in >> k >> bits >> hashes));
    std::vector<Sequence> reads;
    std::string line;
    while (in >> line) reads.emplace_back(line);
    std::ifstream qin(ask_path);
    std::vector<uint64_t> ask;
    uint64_t v;
    while (qin >> v) ask.push_back(v);
    if (k == 16) run_file<Kmer16b32bit>(reads, uint8_t(k), bits, hashes, ask);
    else run_file<Kmer64bit>(reads, uint8_t(k), bits, hashes, ask);
}

}  // namespace

int main(int argc, char **argv) {
    try {
        test_by_hand();
        if (argc > 2) test_files(argv[1], argv[2]);
        std::printf("ok test_kfilter\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_kfilter: %s\n", e.what());
        return 1;
    }
}

// test_read_stats -- the read statistics of the C++ mirror (include/kmerutils.hpp: ReadBaseDistribution, get_base_count_par, the two
// dumps, remap_quality8, ingest_fastq_qual, read_quality_stats).  The host-only pieces are checked here; then a context is made
// (without a device the program stops with the library's error, "no CPU fallback"), and given a FASTQ file and a directory the
// program ingests the text with its qualities, prints the reads' quality bytes, the percentage table, the non-empty length
// buckets, the totals and the quality records, and writes bases.histo and readlen.histo into the directory;
// tests/test_cpp_read_stats.py compares all of it with the numpy model.
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

void test_host_only() {
    CHECK(rust_display(0.) == "0" && rust_display(1.) == "1" && rust_display(0.5) == "0.5" && rust_display(1. / 3) == "0.3333333333333333");
    CHECK(rust_display(1. / 3e6) == "0.00000033333333333333335" && rust_display(100.) == "100");
    const uint8_t edges[] = {0x00, 0x24, 0x25, 0x27, 0x28, 0x36, 0x37, 0x38, 0xFF}, want[] = {0, 0, 1, 1, 2, 6, 7, 7, 7};
    for (int i = 0; i < 9; i++) CHECK(remap_quality8(edges[i]) == want[i]);
    uint32_t n_buckets = 0;
    uint64_t limit = 0, lo = 0, hi = 0;
    CHECK(kmu_len_hist_layout(1000000, 3, &n_buckets, &limit) == KMU_OK && n_buckets == 11264 && limit == 1048576);
    CHECK(kmu_len_bucket_range(3, 2048 + 476, &lo, &hi) == KMU_OK && lo == 3000 && hi == 3001);
    // the quantile and the refusal of a short histogram need no device either
    std::vector<uint64_t> hist(n_buckets, 0);
    hist[5] = 3;
    hist[2048 + 476] = 1;
    const ReadBaseDistribution d(std::vector<uint64_t>(404, 0), hist, 4, 0, 0, 1000000, 3);
    CHECK(d.value_at_quantile(0.) == 5 && d.value_at_quantile(0.75) == 5 && d.value_at_quantile(0.76) == 3001 && d.value_at_quantile(1.) == 3001);
    CHECK(d.ascii_dump_readlen_distribution("/nonexistent-directory/readlen.histo") == "histogram error!");
}

void test_by_hand(Context &ctx) {
    const std::string text = "@a\nAAAAAAAA\n+\n!!!!IIII\n@n\nACNT\n+\nIIII\n@b\nACGTACGA\r\n+\r\n%%%%((((\r\n@c\nGGGT\n+\n7777";
    const FastqQualReads r = ingest_fastq_qual(reinterpret_cast<const uint8_t *>(text.data()), text.size(), ctx);
    CHECK(r.info.n_records == 4 && r.info.n_kept == 3 && r.info.kept_bases == 20 && r.info.nb_bad_reads == 1);
    CHECK(std::string(r.bases.begin(), r.bases.begin() + 20) == "AAAAAAAAACGTACGAGGGT");
    CHECK(std::string(r.quals.begin(), r.quals.begin() + 20) == "!!!!IIII%%%%((((7777");
    const FastqReads plain = parse_fastq_text(reinterpret_cast<const uint8_t *>(text.data()), text.size(), ctx);
    CHECK(plain.offsets == r.offsets && std::equal(plain.bases.begin(), plain.bases.begin() + 20, r.bases.begin()));
    const ReadBaseDistribution d = get_base_count_par(batch_of(r, 0, 3), 1000000, 3, ctx);
    CHECK(d.nb_reads == 3 && d.histo_out == 0 && d.non_acgt == 0 && d.readsize_len() == 3 && d.len_hist[8] == 2 && d.len_hist[4] == 1);
    CHECK(d.acgt_distribution[100 * 4 + 0] == 1. / 3 && d.acgt_distribution[38 * 4 + 0] == 1. / 3 && d.acgt_distribution[0 * 4 + 0] == 1. / 3);
    const ReadQualityStats q = read_quality_stats(std::vector<uint8_t>(r.quals.begin(), r.quals.begin() + 20), r.offsets, ctx);
    CHECK(q.reads.size() == 3 && q.reads[0].n_class[0] == 4 && q.reads[0].n_class[7] == 4 && q.reads[0].median_class == 0);
    CHECK(q.reads[0].min_q == '!' && q.reads[0].max_q == 'I' && q.reads[0].sum_q == 4 * uint64_t('!') + 4 * uint64_t('I'));
    CHECK(q.reads[1].n_class[1] == 4 && q.reads[1].n_class[2] == 4 && q.reads[1].median_class == 1 && q.reads[2].n_class[7] == 4);
    CHECK(q.class_hist[0] == 4 && q.class_hist[1] == 4 && q.class_hist[2] == 4 && q.class_hist[7] == 8);
    bool refused = false;
    const std::string bad = "@a\nACGT\n+\nIII\n";
    try {
        (void) ingest_fastq_qual(reinterpret_cast<const uint8_t *>(bad.data()), bad.size(), ctx);
    } catch (const KmuError &e) {
        refused = e.status() == KMU_E_BAD_ARG && std::string(e.what()).find("invalid record") != std::string::npos;
    }
    CHECK(refused);
}

void test_file(Context &ctx, const char *fastq_path, const std::string &outdir) {
    std::ifstream in(fastq_path, std::ios::binary);
    const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    const FastqQualReads r = ingest_fastq_qual(reinterpret_cast<const uint8_t *>(text.data()), text.size(), ctx);
    std::printf("kept %llu %llu\n", (unsigned long long) r.info.n_kept, (unsigned long long) r.info.kept_bases);
    for (size_t i = 0; i < r.nb_reads(); i++) {
        std::printf("read %llu ", (unsigned long long) (r.offsets[i + 1] - r.offsets[i]));
        for (uint64_t p = r.offsets[i]; p < r.offsets[i + 1]; p++) std::printf("%02x", r.quals[p]);
        std::printf("\n");
    }
    const ReadBaseDistribution d = get_base_count_par(batch_of(r, 0, r.nb_reads()), 1000000, 3, ctx);
    std::printf("totals %llu %llu %llu\n", (unsigned long long) d.nb_reads, (unsigned long long) d.histo_out, (unsigned long long) d.non_acgt);
    for (size_t b = 0; b < d.len_hist.size(); b++)
        if (d.len_hist[b]) std::printf("len %zu %llu\n", b, (unsigned long long) d.len_hist[b]);
    d.ascii_dump_acgt_distribution(outdir + "/bases.histo");
    const std::string err = d.ascii_dump_readlen_distribution(outdir + "/readlen.histo");
    std::printf("readlen_error %d\n", err.empty() ? 0 : 1);
    const ReadQualityStats q = read_quality_stats(std::vector<uint8_t>(r.quals.begin(), r.quals.begin() + r.info.kept_bases), r.offsets, ctx);
    for (const kmu_read_qual &x : q.reads) {
        std::printf("qual");
        for (uint64_t c : x.n_class) std::printf(" %llu", (unsigned long long) c);
        std::printf(" %llu %u %u %u\n", (unsigned long long) x.sum_q, unsigned(x.min_q), unsigned(x.max_q), unsigned(x.median_class));
    }
    std::printf("classes");
    for (uint64_t c : q.class_hist) std::printf(" %llu", (unsigned long long) c);
    std::printf("\nend\n");
}

}  // namespace

int main(int argc, char **argv) {
    try {
        test_host_only();
        Context ctx(0);
        test_by_hand(ctx);
        if (argc > 2) test_file(ctx, argv[1], argv[2]);
        std::printf("ok test_read_stats\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_read_stats: %s\n", e.what());
        return 1;
    }
}

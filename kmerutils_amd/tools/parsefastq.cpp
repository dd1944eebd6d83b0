// parsefastq -f reads.fastq [--stats] [kmer (--count -s <kmer size> [--repeated [--filter-bits n]] | --unique)] [-t threads] [-b 2]
//            [--outdir dir] [--device n] [--histo file]
//
// The counting branch of the reference's tool (src/bin/parsefastq.rs:215-236: `kmer --count`) on the GPU path: the FASTQ
// text is filtered on the device like parse_with_needletail does on the host (src/io.rs:37-57), every canonical k-mer of
// the accepted reads is counted (count_kmer_threaded_one_to_many, src/base/kmercount.rs:881-974) and the k-mers seen at
// least twice are written as a COUNTER_MULTIPLE dump to <fastq>.multi_kmer.bin (kmercount.rs:467-531).  `--unique` is the
// Unicity branch (parsefastq.rs:238-247): the 16-mers seen exactly once, with (sequence, position), to <fastq>.once_kmer.bin.
// `--histo <file>` (with --count; no counterpart upstream): the count spectrum of the table, one `count<TAB>number of distinct
// k-mers` line per non-empty bin, ascending (counts saturate at 255).
// `--repeated` (with --count; no counterpart upstream): the count through the Bloom prefilter (count_repeated_kmers) -- two passes
// over the reads, the k-mers seen once stay off the table; the dump is byte for byte that of the plain count, counts >= 2 being
// exact either way.  `--filter-bits <n>`: filter bits per k-mer occurrence (default 16).  `--histo` is refused with it: the table
// holds no singletons, bin 1 would be meaningless.
// `--stats` is what the reference's tool does before it counts (parsefastq.rs:193-203): get_base_count_par(reads, 1000000, 3), then
// bases.histo and readlen.histo in --outdir (the refusal of fewer than 100 reads is discarded, as upstream), and for a FASTQ text
// quality.histo, eight lines `class<TAB>number of bases` of the kept reads' qualities (remap_quality8).  Off by default: a run without
// it writes what it always wrote.  It needs no `kmer` task: `parsefastq -f reads.fastq --stats` writes the statistics alone.
// Kmer type by size as upstream: k <= 14 Kmer32bit, k == 16 Kmer16b32bit, else Kmer64bit (k <= 31).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/kmerutils.hpp"

using namespace kmerutils;

static void usage() {
    std::fprintf(stderr, "usage: parsefastq -f <fastq> [--stats] [kmer (--count -s <kmer size> [--repeated [--filter-bits <n>]] | --unique)] "
                         "[-t <threads>] [-b 2] [--outdir <dir>] [--device <n>] [--histo <file>]\n");
    std::exit(2);
}

// parsefastq.rs:193-203, and the quality classes where the text had quality lines
static void write_stats(const DeviceReads &reads, const std::string &outdir, Context &ctx) {
    const ReadBaseDistribution dist = get_base_count_par(reads.batch(0, reads.nb_reads()), 1000000, 3, ctx);
    std::fprintf(stderr, "nb read outside max size for histogram %llu\n", (unsigned long long) dist.histo_out);   // statutils.rs:338-341
    dist.ascii_dump_acgt_distribution(outdir + "/bases.histo");
    (void) dist.ascii_dump_readlen_distribution(outdir + "/readlen.histo");
    if (!reads.has_quals()) return;
    const ReadQualityStats q = read_quality_stats(reads.quals_batch(0, reads.nb_reads()), false, ctx);
    std::FILE *f = std::fopen((outdir + "/quality.histo").c_str(), "w");
    if (!f) throw std::runtime_error("cannot write " + outdir + "/quality.histo");
    for (size_t c = 0; c < q.class_hist.size(); c++) std::fprintf(f, "%zu\t%llu\n", c, (unsigned long long) q.class_hist[c]);
    std::fclose(f);
}

template <class Kmer>
static void count_repeated_and_dump(const DeviceReads &reads, uint8_t kmer_size, uint32_t filter_bits, const std::string &dumpfname, Context &ctx) {
    RepeatedKmers<Kmer> r = count_repeated_kmers<Kmer>(reads.batch(0, reads.nb_reads()), kmer_size, 8, filter_bits, 4, 0, ctx);
    const kmu_kfilter_info_t fi = r.filter->info();
    std::fprintf(stderr, " prefilter: %llu of %llu kmer occurrences passed, filter bytes %llu, estimated distinct %.0f\n",
                 (unsigned long long) r.nb_passed, (unsigned long long) fi.n_added, (unsigned long long) fi.bytes, fi.est_distinct);
    std::fprintf(stderr, " nb distinct kmers held %llu, of which seen once %llu\n", (unsigned long long) r.counter->get_nb_distinct(),
                 (unsigned long long) r.counter->get_nb_unique());
    const size_t n = r.counter->dump_kmer_counter(dumpfname);
    std::fprintf(stderr, " dumped %zu kmers seen at least twice in %s\n", n, dumpfname.c_str());
}

template <class Kmer>
static void count_and_dump(const DeviceReads &reads, uint8_t kmer_size, const std::string &dumpfname, const std::string &histofname, Context &ctx) {
    KmerCounterPool<Kmer> pool(std::max<uint64_t>(reads.info.kept_bases, 1024), 8, ctx);
    pool.counter().insert_reads(reads.batch(0, reads.nb_reads()), kmer_size);
    std::fprintf(stderr, " nb distinct kmers %llu, nb unique kmers %llu\n", (unsigned long long) pool.get_nb_distinct(),
                 (unsigned long long) pool.get_nb_unique());
    const size_t n = pool.dump_kmer_counter(dumpfname);
    std::fprintf(stderr, " dumped %zu kmers seen at least twice in %s\n", n, dumpfname.c_str());
    if (!histofname.empty()) {
        const std::vector<uint64_t> h = pool.counter().get_count_histogram();
        std::FILE *f = std::fopen(histofname.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + histofname);
        for (size_t v = 0; v < h.size(); v++)
            if (h[v]) std::fprintf(f, "%zu\t%llu\n", v, (unsigned long long) h[v]);
        std::fclose(f);
    }
}

int main(int argc, char **argv) {
    std::string fname, outdir = ".", histo;
    long kmer_size = 0, device = 0, filter_bits = 16;
    bool count = false, kmer_cmd = false, unique = false, repeated = false, stats = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> const char * {
            if (i + 1 >= argc) usage();
            return argv[++i];
        };
        if (a == "-f" || a == "--file") fname = next();
        else if (a == "kmer") kmer_cmd = true;
        else if (a == "--count") count = true;
        else if (a == "--unique" || a == "-u") unique = true;
        else if (a == "-s" || a == "--size") kmer_size = std::atol(next());
        else if (a == "-t" || a == "--threads") next();   // accepted: the device needs no thread count
        else if (a == "-b" || a == "--bits") {
            if (std::atol(next()) != 2) {
                std::fprintf(stderr, "k-mers need 2 bits per base (kmergenerator.rs:221-223)\n");
                return 2;
            }
        } else if (a == "--outdir") outdir = next();
        else if (a == "--device") device = std::atol(next());
        else if (a == "--histo") histo = next();
        else if (a == "--repeated") repeated = true;
        else if (a == "--stats") stats = true;
        else if (a == "--filter-bits") filter_bits = std::atol(next());
        else usage();
    }
    const bool stats_alone = stats && !kmer_cmd && !count && !unique;
    if (fname.empty() || (!stats_alone && (!kmer_cmd || (!count && !unique))) || (count && (kmer_size < 1 || kmer_size > 31))) usage();
    if (repeated && (!count || unique || filter_bits < 1)) usage();
    if (repeated && !histo.empty()) {
        std::fprintf(stderr, "--histo with --repeated: the table holds no singletons, bin 1 would be meaningless\n");
        return 2;
    }
    try {
        const auto t0 = std::chrono::steady_clock::now();
        Context ctx{int(device)};
        DeviceReads reads = stats ? DeviceReads::from_file_qual(fname, ctx) : DeviceReads::from_file(fname, ctx);
        std::fprintf(stderr, " nb reads %llu, nb bases %llu, nb bad bases %llu, nb reads with non acgt %llu\n",
                     (unsigned long long) reads.info.n_records, (unsigned long long) reads.info.n_bases,
                     (unsigned long long) reads.info.nb_bad_bases, (unsigned long long) reads.info.nb_bad_reads);
        if (stats) write_stats(reads, outdir, ctx);
        // the tool writes <basename>.multi_kmer.bin into the working directory (parsefastq.rs:207-211)
        const size_t slash = fname.rfind('/');
        const std::string dumpfname = outdir + "/" + (slash == std::string::npos ? fname : fname.substr(slash + 1)) + ".multi_kmer.bin";
        if (stats_alone) {   // no k-mer task: the statistics were all there was to do
        } else if (unique) {   // KmerProcessing::Unicity (parsefastq.rs:238-247): filter1_kmer_16b32bit + the once-k-mer dump
            KmerFilter1 filter(16, uint32_t(std::min<uint64_t>(std::max<uint64_t>(reads.info.kept_bases, 1024), 0xFFFFFFFFu)), ctx);
            detail::Batch all = reads.batch(0, reads.nb_reads());
            filter.insert_reads(all);
            const std::string oncefname = outdir + "/" + (slash == std::string::npos ? fname : fname.substr(slash + 1)) + ".once_kmer.bin";
            std::fprintf(stderr, "dumping unique kmers in file : %s \n", oncefname.c_str());
            const size_t n = filter.dump_in_file_once_kmer16b32bit(oncefname, all);
            std::fprintf(stderr, "dump_in_file_once_kmer16b32bit, number of kmer dumped : %zu (distinct once-k-mers %llu)\n", n,
                         (unsigned long long) filter.get_nb_once());
        } else if (repeated) {
            if (kmer_size <= 14) count_repeated_and_dump<Kmer32bit>(reads, uint8_t(kmer_size), uint32_t(filter_bits), dumpfname, ctx);
            else if (kmer_size == 16) count_repeated_and_dump<Kmer16b32bit>(reads, uint8_t(kmer_size), uint32_t(filter_bits), dumpfname, ctx);
            else count_repeated_and_dump<Kmer64bit>(reads, uint8_t(kmer_size), uint32_t(filter_bits), dumpfname, ctx);
        } else if (kmer_size <= 14) count_and_dump<Kmer32bit>(reads, uint8_t(kmer_size), dumpfname, histo, ctx);
        else if (kmer_size == 16) count_and_dump<Kmer16b32bit>(reads, uint8_t(kmer_size), dumpfname, histo, ctx);
        else count_and_dump<Kmer64bit>(reads, uint8_t(kmer_size), dumpfname, histo, ctx);
        std::fprintf(stderr, " elapsed time (s) %.3f\n",
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    } catch (const std::exception &e) {
        std::fprintf(stderr, "parsefastq: %s\n", e.what());
        return 1;
    }
    return 0;
}

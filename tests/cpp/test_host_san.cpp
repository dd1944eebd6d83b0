// Host-only code of include/kmerutils.hpp under AddressSanitizer + UndefinedBehaviorSanitizer (`make sanitize`; no GPU, no
// libkmu call): packed sequences, k-mer values, parameter files, the signature dump writer / reader, the k-mer count reloader,
// the chunk plan of kmu_sketch_count's host pipeline (kmerutils_amd/csrc/kmu_pipe_plan.hpp) and the plans of the partitioned
// count build (kmerutils_amd/csrc/kmu_count_plan.hpp): host arithmetic of libkmu.
// The reference leans on Rust ownership and bounds checks for these (src/base/sequence.rs, src/sketching/seqsketchjaccard.rs:385-712,
// src/base/kmercount.rs:1148-1503); this side is C++ and gets the sanitizers instead.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../include/kmerutils.hpp"
#include "../../kmerutils_amd/csrc/kmu_count_plan.hpp"
#include "../../kmerutils_amd/csrc/kmu_pipe_plan.hpp"

using namespace kmerutils;

static int failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        if (!(x)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } \
    } while (0)

static std::string random_dna(std::mt19937_64 &rng, size_t n, bool mixed_case) {
    std::string s(n, 'A');
    for (auto &c : s) {
        c = "ACGT"[rng() & 3];
        if (mixed_case && (rng() & 1)) c = char(c + 32);
    }
    return s;
}
static std::string upper(std::string s) {
    for (auto &c : s) c = char(std::toupper((unsigned char) c));
    return s;
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : "/tmp";
    std::mt19937_64 rng(0x5A17);
    // ---- Sequence::new(raw, 2), sequence.rs:25-106: every length around the byte and word edges ----
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(4), size_t(5), size_t(15), size_t(16), size_t(17), size_t(63), size_t(64), size_t(65), size_t(1000), size_t(4097)}) {
        const std::string s = random_dna(rng, n, true);
        Sequence q(s);
        CHECK(q.size() == n && q.compressed_length() == (n + 3) / 4);
        const auto d = q.decompress();
        CHECK(std::string(d.begin(), d.end()) == upper(s));
        const auto rr = q.get_reverse_complement().get_reverse_complement().decompress();
        CHECK(std::string(rr.begin(), rr.end()) == upper(s));
        if (n) CHECK(q.get_base(n - 1) == Alphabet2b::encode(uint8_t(s[n - 1])));
    }
    {
        bool threw = false;
        try { Sequence bad(std::string("ACGNT")); } catch (const std::invalid_argument &) { threw = true; }
        CHECK(threw);  // Alphabet2b::encode panics upstream (alphabet.rs:125)
    }
    // ---- k-mer values: push = shift in, reverse_complement an involution, min the canonical form ----
    for (int k = 1; k <= 14; k++) {
        Kmer32bit a = Kmer32bit::build(0, uint8_t(k));
        const std::string s = random_dna(rng, size_t(k) + 7, false);
        for (char c : s) a = a.push(Alphabet2b::encode(uint8_t(c)));
        const auto u = a.get_uncompressed_kmer();
        CHECK(std::string(u.begin(), u.end()) == s.substr(s.size() - size_t(k)));
        CHECK(a.reverse_complement().reverse_complement() == a && a.get_nb_base() == k);
        CHECK(!(a.reverse_complement().min(a) == a) || !(a.reverse_complement() < a));
    }
    {
        Kmer16b32bit a;
        const std::string s = random_dna(rng, 40, false);
        for (char c : s) a = a.push(Alphabet2b::encode(uint8_t(c)));
        const auto u = a.get_uncompressed_kmer();
        CHECK(std::string(u.begin(), u.end()) == s.substr(24) && a.reverse_complement().reverse_complement() == a);
    }
    for (int k = 1; k <= 31; k++) {
        Kmer64bit a = Kmer64bit::build(0, uint8_t(k));
        const std::string s = random_dna(rng, size_t(k) + 11, false);
        for (char c : s) a = a.push(Alphabet2b::encode(uint8_t(c)));
        const auto u = a.get_uncompressed_kmer();
        CHECK(std::string(u.begin(), u.end()) == s.substr(s.size() - size_t(k)));
        CHECK(a.reverse_complement().reverse_complement() == a);
    }
    // ---- parameter files (sketcharg.rs:40-138) ----
    {
        SeqSketcherParams p(21, 400, SketchAlgo(1), DataType(0));
        p.dump_json(dir + "/sketchparams_dump.json");
        const SeqSketcherParams r = SeqSketcherParams::reload_json(dir);
        CHECK(r.get_kmer_size() == 21 && r.get_sketch_size() == 400 && int(r.get_algo()) == 1 && int(r.get_data_t()) == 0);
        bool threw = false;
        try { (void) SeqSketcherParams::reload_json(dir + "/no_such_dir"); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
        std::ofstream(dir + "/sketchparams_dump.json") << "{\"kmer_size\":8";  // truncated: a field is missing
        threw = false;
        try { (void) SeqSketcherParams::reload_json(dir); } catch (const std::exception &) { threw = true; }
        CHECK(threw);
    }
    // ---- the signature dump (seqsketchjaccard.rs:385-414, 572-583) and its reader (:586-712), incl. a truncated last row ----
    {
        const std::string f = dir + "/sigs.bin";
        const size_t m = 37, rows = 11;
        std::vector<std::vector<uint32_t>> sig(rows, std::vector<uint32_t>(m));
        for (auto &r : sig) for (auto &v : r) v = uint32_t(rng());
        {
            std::ofstream out(f, std::ios::binary);
            const uint32_t head[4] = {SeqSketcher::MAGIC_SIG_DUMP, 4u, uint32_t(m), 8u};
            out.write(reinterpret_cast<const char *>(head), sizeof head);
            SeqSketcher::dump_signatures_block_u32(sig, out);
            std::vector<uint32_t> flat;
            for (const auto &r : sig) flat.insert(flat.end(), r.begin(), r.end());
            SeqSketcher::dump_signatures_block_u32(flat, flat.size(), out);
            out.write("xyz", 3);  // a partial row at the end
        }
        SigSketchFileReader rd(f);
        CHECK(rd.get_kmer_size() == 8 && rd.get_signature_length() == m && rd.get_signature_size() == 4);
        size_t n = 0;
        while (auto row = rd.next()) { CHECK(*row == sig[n % rows]); n++; }
        CHECK(n == 2 * rows);
        std::ofstream(f, std::ios::binary).write("\xdd\xea", 2);  // two bytes: no magic
        bool threw = false;
        try { SigSketchFileReader bad(f); } catch (const std::runtime_error &) { threw = true; }
        CHECK(threw);
    }
    // ---- k-mer count dumps (kmercount.rs:1148-1503): both record widths, a truncated record, a wrong magic ----
    for (uint8_t nbc : {uint8_t(1), uint8_t(2)}) {
        const std::string f = dir + "/counts.bin";
        std::vector<std::pair<uint32_t, uint16_t>> recs;
        for (int i = 0; i < 1000; i++) recs.emplace_back(uint32_t(rng()), uint16_t(rng() & (nbc == 1 ? 0xFF : 0xFFFF)));
        {
            std::ofstream out(f, std::ios::binary);
            const uint32_t magic = 0xcea2bbff;
            const uint8_t k = 16;
            const uint64_t n = recs.size();
            out.write(reinterpret_cast<const char *>(&magic), 4); out.write(reinterpret_cast<const char *>(&k), 1);
            out.write(reinterpret_cast<const char *>(&nbc), 1); out.write(reinterpret_cast<const char *>(&n), 8);
            for (auto &r : recs) { out.write(reinterpret_cast<const char *>(&r.first), 4); out.write(reinterpret_cast<const char *>(&r.second), nbc); }
            out.write("\x01\x02", 2);  // half a record
        }
        auto r = KmerCountReload::load_multiple_kmers_from_file(f);
        CHECK(r && r->get_kmer_size() == 16 && r->get_nb_kmer() == recs.size() && r->kmers().size() == recs.size());
        auto c = r ? r->get_multi_kmer_counts() : std::nullopt;
        CHECK(c && c->size() == recs.size() && (*c)[999] == recs[999].second && r->kmers()[0] == recs[0].first);
        CHECK(!r->get_coord_from_rank(0));
        CHECK(KmerCountReload::load_unique_kmer_from_file(f) == nullptr);  // the other dump's magic
        CHECK(KmerCountReload::load_multiple_kmers_from_file(dir + "/missing.bin") == nullptr);
    }
    {
        const std::string f = dir + "/unique.bin";
        {
            std::ofstream out(f, std::ios::binary);
            const uint32_t magic = 0xcea2bbdd;
            const uint8_t k = 16;
            const uint64_t n = 3;
            out.write(reinterpret_cast<const char *>(&magic), 4); out.write(reinterpret_cast<const char *>(&k), 1); out.write(reinterpret_cast<const char *>(&n), 8);
            for (uint32_t i = 0; i < 3; i++) { const uint32_t rec[3] = {100 + i, i, 7 * i}; out.write(reinterpret_cast<const char *>(rec), 12); }
        }
        auto r = KmerCountReload::load_unique_kmer_from_file(f);
        CHECK(r && r->kmers().size() == 3 && !r->get_multi_kmer_counts());
        auto p = r ? r->get_coord_from_rank(2) : std::nullopt;
        CHECK(p && !r->get_coord_from_rank(3));
    }
    // ---- the chunk plan of kmu_sketch_count's host pipeline (kmu_pipe_plan.hpp) ----
    {
        using kmu::pipe_chunk_plan;
        std::vector<uint32_t> cut;
        std::vector<uint64_t> pk;
        auto offsets_of = [](const std::vector<uint64_t> &len) {
            std::vector<uint64_t> h(1, 0);
            for (uint64_t l : len) h.push_back(h.back() + l);
            return h;
        };
        // random read-length sets: empty reads, a single read longer than every target, n_seq of 0 and 1, growth 1 and 3
        for (int it = 0; it < 4000; it++) {
            const uint32_t n_seq = it < 40 ? uint32_t(it & 1) : uint32_t(rng() % 60);
            std::vector<uint64_t> len(n_seq);
            for (auto &l : len) l = rng() % 4 == 0 ? 0 : rng() % (1 + rng() % 6000);
            if (n_seq && it % 5 == 0) len[rng() % n_seq] = 200000 + rng() % 100000;  // longer than every target below
            const std::vector<uint64_t> h = offsets_of(len);
            const uint64_t total = h[n_seq], chunk = 1 + rng() % 20000, growth = it & 2 ? 3 : 1;
            pipe_chunk_plan(h, n_seq, total, chunk, growth, true, &cut, &pk);
            CHECK(!cut.empty() && cut.front() == 0 && cut.back() == n_seq);
            for (size_t c = 0; c + 1 < cut.size(); c++) CHECK(cut[c] < cut[c + 1]);
            const size_t n_chunks = cut.size() - 1;
            CHECK(n_chunks ? pk.size() == n_chunks + 1 : pk.empty());
            if (n_chunks) CHECK(pk.front() == 0 && pk.back() == total);
            for (size_t c = 0; c < n_chunks; c++) {
                CHECK(pk[c] <= pk[c + 1]);
                if (c + 1 < n_chunks) CHECK(pk[c + 1] % 16 == 0 || pk[c + 1] == total);
                CHECK(pk[c + 1] >= std::min(total, h[cut[c + 1]]));
            }
            pipe_chunk_plan(h, n_seq, total, chunk, growth, false, &cut, &pk);
            CHECK(pk.empty() && cut.back() == n_seq);
        }
        // the headline's 4.38 G bases as 438 000 reads of 10 000, 512 MiB chunks, growth 3: 64 MiB, 192 MiB, 576 MiB, 1 728 MiB and the
        // rest, each ended at the first read boundary at or behind its target
        std::vector<uint64_t> h(438000 + 1);
        for (size_t i = 0; i < h.size(); i++) h[i] = i * 10000ull;
        pipe_chunk_plan(h, 438000, h.back(), 512ull << 20, 3, true, &cut, &pk);
        CHECK(cut.size() == 6);
        uint64_t target = 0;
        for (size_t c = 0; c + 2 < cut.size(); c++) {
            const uint64_t mib[4] = {64, 192, 576, 1728};
            target += mib[c] << 20;
            CHECK(h[cut[c + 1]] >= target && h[cut[c + 1] - 1] < target);
        }
        // expected values generated once from the lines this function was taken from (kmu_sketch.hip before the split)
        CHECK((cut == std::vector<uint32_t>{0u, 6711u, 26844u, 87242u, 268436u, 438000u}));
        CHECK((pk == std::vector<uint64_t>{0ull, 67110000ull, 268440000ull, 872420000ull, 2684360000ull, 4380000000ull}));
        pipe_chunk_plan(h, 438000, h.back(), 512ull << 20, 1, false, &cut, &pk);
        CHECK((cut == std::vector<uint32_t>{0u, 6711u, 60623u, 114534u, 168445u, 222356u, 276267u, 330178u, 384089u, 438000u}) && pk.empty());
        const std::vector<uint64_t> s = offsets_of({700, 0, 1300, 50, 0, 9000, 10, 10, 10, 400, 2500, 0, 1});
        pipe_chunk_plan(s, 13, s.back(), 8192, 3, true, &cut, &pk);
        CHECK((cut == std::vector<uint32_t>{0u, 3u, 6u, 13u}) && (pk == std::vector<uint64_t>{0ull, 2000ull, 11056ull, 13981ull}));
        pipe_chunk_plan(s, 13, s.back(), 4096, 1, true, &cut, &pk);
        CHECK((cut == std::vector<uint32_t>{0u, 1u, 6u, 7u, 13u}) && (pk == std::vector<uint64_t>{0ull, 704ull, 11056ull, 11072ull, 13981ull}));
        pipe_chunk_plan(s, 13, s.back(), 2048, 2, false, &cut, &pk);
        CHECK((cut == std::vector<uint32_t>{0u, 1u, 3u, 4u, 6u, 7u, 13u}) && pk.empty());
    }
    // ---- the plans of the partitioned count build (kmu_count_plan.hpp) ----
    {
        using namespace kmu;
        CHECK(flat_wave_steps(0) == 0 && flat_wave_steps(1) == 1 && flat_wave_steps(1024) == 1 && flat_wave_steps(1025) == 2);
        // the unit split: every step in exactly one unit, no unit without a step, no more units than the cap
        for (uint64_t cap : {uint64_t(256), uint64_t(2048)})
            for (uint64_t nsteps : {uint64_t(0), uint64_t(1), uint64_t(2), cap - 1, cap, cap + 1, 3 * cap + 1, uint64_t(1) << 33}) {
                const UnitSplit u = unit_split(nsteps, cap);
                const uint64_t n = std::max<uint64_t>(nsteps, 1);
                CHECK(u.units >= 1 && u.units <= cap && u.asked == std::min(n, cap));
                CHECK((uint64_t) u.units * u.steps_per_unit >= n && n > (uint64_t) (u.units - 1) * u.steps_per_unit);
            }
        // stream capacities: whole 128-byte lines, never below mean + 5 sigma + 32 at the full share, monotone in the mean
        uint64_t prev = 0;
        for (double mean = 0.0; mean < 3e9; mean = mean * 1.37 + 0.61) {
            const uint64_t cap = seg_cap_for(mean, 1.0);
            CHECK(cap % 16 == 0 && (double) cap >= mean + 5.0 * std::sqrt(mean) + 32.0 && cap >= prev);
            CHECK(seg_cap_for(mean, 0.6) % 16 == 0 && seg_cap_for(mean, 0.6) <= cap);
            prev = cap;
        }
        for (uint32_t cus : {1u, 2u, 15u, 16u, 17u, 256u})
            for (uint64_t bases : {uint64_t(0), uint64_t(1), uint64_t(1024), uint64_t(16 * 1024 + 1), uint64_t(300000), uint64_t(4380000000ull)}) {
                const SegPlan sp = seg_plan(cus, bases, 128, 40, 1.0);
                const UnitSplit u = unit_split(flat_wave_steps(bases), cus);
                CHECK(sp.units1 == u.units && sp.steps_per_unit == u.steps_per_unit);
                CHECK(sp.sets >= 1 && sp.sets <= std::min(16u, sp.units1) && sp.cap1 % 16 == 0 && sp.cap2 % 16 == 0);
                const SegPlan sa = seg_plan_array(cus, bases, 128, 40, 1.0);
                CHECK(sa.units1 == cus && sa.sets == std::min(16u, cus) && sa.cap1 >= (uint64_t) ((double) bases / sa.sets / 128));
            }
        // the headline's level 1 (256 CUs, 4.38 G bases, 2^11 groups): expected values from the lines this was taken from
        {
            const SegPlan sp = seg_plan(256, 4380000000ull, 2048, 1024, 1.0);
            CHECK(sp.units1 == 256 && sp.steps_per_unit == 16709 && sp.sets == 16 && sp.cap1 == 135536 && sp.cap2 == 2352);
        }
        // 2^bits leaves as 2^b1 groups of n2
        for (int bits = 0; bits <= 22; bits++) {
            int b1 = -1;
            uint32_t n2 = 0;
            region_split(bits, &b1, &n2);
            CHECK(((uint64_t) 1 << b1) * n2 == (uint64_t) 1 << bits && b1 >= 0 && b1 <= 11 && n2 <= 2048 && (b1 == 0) == (bits <= 11));
        }
        // the rounds of level 1 under an upload: random arrivals (repeats, a jump straight to the end), unit counts and minima
        for (int it = 0; it < 20000; it++) {
            const uint64_t total = it < 50 ? uint64_t(it) : rng() % (it % 7 == 0 ? 5000000 : 70000);
            const uint32_t units1 = 1 + uint32_t(rng() % 300);
            const uint64_t min_per_unit = rng() % 3 == 0 ? 0 : rng() % 70, nsteps = flat_wave_steps(total);
            uint64_t ready = 0, done = 0;
            bool finished = false;
            for (int call = 0; call < 1000 && !finished; call++) {
                const uint64_t r = rng() % 8;
                if (r == 0) ready = total;                                       // straight to the end
                else if (r > 2) ready = std::min(total, ready + rng() % (total / 3 + 2)); // (else: the same value again)
                if (call == 999) ready = total;
                const SegRound sr = seg_round(total, ready, done, units1, min_per_unit);
                CHECK(sr.launch == (sr.n_new != 0) && sr.last == (ready >= total));
                if (sr.n_new) CHECK(sr.last || sr.n_new >= (uint64_t) units1 * min_per_unit);
                if (!sr.last) CHECK(sr.n_new == 0 || (ready >= 32 && (done + sr.n_new) * 1024 <= ready - 32));
                done += sr.n_new; // the launched ranges are [done, done + n_new): in order, no gap, no overlap
                CHECK(done <= nsteps);
                finished = sr.last;
            }
            CHECK(finished && done == nsteps); // the last call completes whatever was held back
            const SegRound after = seg_round(total, total, done, units1, min_per_unit);
            CHECK(!after.launch && after.n_new == 0);
        }
    }
    std::printf("%s: %d failure(s)\n", argv[0], failures);
    return failures ? 1 : 0;
}

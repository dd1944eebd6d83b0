// test_anchor_index -- AnchorIndex of the C++ mirror (include/kmerutils.hpp) against a brute force written here: rows drawn from a
// small pool of hashes, one hash carried by a third of the database rows, so that a repeat mask has something to drop; info() and
// occupancy() against a std::map of the database keys; match_read_anchors with a mask nothing reaches against the call without one.
// Without a device it stops with the library's error ("no CPU fallback").
#include <cstdio>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <tuple>

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

uint64_t next(uint64_t &state) {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return state >> 33;
}

// `rows` bottom-k rows of length m over a pool of `pool` hashes; every third row also holds `hot`, smaller than the whole pool
std::vector<uint64_t> make_rows(uint64_t &state, uint32_t rows, uint32_t m, uint32_t pool, uint64_t hot) {
    std::vector<uint64_t> h(size_t(rows) * m, UINT64_MAX);
    for (uint32_t r = 0; r < rows; r++) {
        std::set<uint64_t> s;
        const uint32_t n = uint32_t(next(state) % (m + 1));
        if (r % 3 == 0 && n > 0) s.insert(hot);
        while (s.size() < n) s.insert(1000 + 7919 * (next(state) % pool));
        size_t t = 0;
        for (uint64_t x : s) h[size_t(r) * m + t++] = x;
    }
    return h;
}

std::vector<uint64_t> row_of(const std::vector<uint64_t> &h, uint32_t r, uint32_t m) {
    std::vector<uint64_t> out;
    for (uint32_t t = 0; t < m && h[size_t(r) * m + t] != UINT64_MAX; t++) out.push_back(h[size_t(r) * m + t]);
    return out;
}

// minhash_distance (minhash.rs:134-190): common, total, i
std::tuple<uint32_t, uint32_t, uint32_t> walk(const std::vector<uint64_t> &a, const std::vector<uint64_t> &b) {
    const uint32_t n1 = uint32_t(a.size()), n2 = uint32_t(b.size());
    uint32_t i = 0, j = 0, common = 0, total = 0;
    while (i < n1 && j < n2) {
        if (a[i] < b[j]) i++;
        else if (b[j] < a[i]) j++;
        else { i++; j++; common++; }
        total++;
        if (total >= n1) break;
    }
    if (total < n1) {
        if (i < n1) total += n1 - i;
        if (j < n1) total += n1 - j;
        if (total > n1) total = n1;
    }
    return {common, total, i};
}

void test_anchor_index() {
    const uint32_t m = 8, n_keys = 4, ndb = 300, nq = 120;
    uint64_t state = 0xA1C;
    const std::vector<uint64_t> hdb = make_rows(state, ndb, m, 150, 5), hq = make_rows(state, nq, m, 150, 5);
    std::vector<uint32_t> gdb(ndb), gq(nq);
    for (uint32_t b = 0; b < ndb; b++) gdb[b] = (b / 2) % 5;
    for (uint32_t a = 0; a < nq; a++) gq[a] = a % 5;

    std::map<uint64_t, uint32_t> occ;
    uint64_t n_entries = 0;
    for (uint32_t b = 0; b < ndb; b++) {
        const auto rb = row_of(hdb, b, m);
        for (size_t t = 0; t < rb.size() && t < n_keys; t++) { occ[rb[t]]++; n_entries++; }
    }
    uint32_t max_occupancy = 0;
    for (const auto &kv : occ) max_occupancy = std::max(max_occupancy, kv.second);
    CHECK(max_occupancy == occ[5] && max_occupancy > 60);

    AnchorIndex index(hdb, ndb, m, n_keys, gdb);
    const kmu_anchor_index_info_t info = index.info();
    CHECK(info.ndb == ndb && info.m == m && info.n_keys == n_keys && info.has_groups == 1);
    CHECK(info.n_entries == n_entries && info.n_distinct == occ.size() && info.max_occupancy == max_occupancy);
    CHECK(info.device_bytes >= uint64_t(ndb) * m * 8);
    for (uint32_t n_bins : {2u, 16u, max_occupancy + 3}) {
        std::vector<uint64_t> want(n_bins, 0);
        for (const auto &kv : occ) want[std::min(kv.second, n_bins - 1)]++;
        CHECK(index.occupancy(n_bins) == want);
    }

    size_t n_unmasked = 0;
    for (uint32_t max_occ : {0u, 20u, max_occupancy}) {  // 20 masks the hot hash and nothing else
        for (uint32_t min_common : {0u, 2u}) {
            std::vector<std::tuple<uint32_t, uint64_t, uint32_t>> want;
            for (uint32_t a = 0; a < nq; a++) {
                const auto ra = row_of(hq, a, m);
                for (uint32_t b = 0; b < ndb; b++) {
                    if (gq[a] == gdb[b]) continue;
                    const auto rb = row_of(hdb, b, m);
                    uint64_t hstar = UINT64_MAX;
                    for (size_t t = 0; t < ra.size() && t < n_keys; t++)
                        for (size_t u = 0; u < rb.size() && u < n_keys; u++)
                            if (ra[t] == rb[u] && !(max_occ > 0 && occ[ra[t]] > max_occ)) hstar = std::min(hstar, ra[t]);
                    if (hstar != UINT64_MAX && std::get<0>(walk(ra, rb)) >= min_common) want.emplace_back(a, hstar, b);
                }
            }
            std::sort(want.begin(), want.end());
            CHECK(!want.empty());
            std::vector<uint32_t> pairs, dist;
            CHECK(index.match(hq, nq, gq, min_common, max_occ, pairs, dist) == want.size());
            for (size_t p = 0; p < want.size(); p++) {
                const uint32_t a = std::get<0>(want[p]), b = std::get<2>(want[p]);
                CHECK(pairs[2 * p] == a && pairs[2 * p + 1] == b);
                const auto d = walk(row_of(hq, a, m), row_of(hdb, b, m));
                CHECK(dist[3 * p] == std::get<0>(d) && dist[3 * p + 1] == std::get<1>(d) && dist[3 * p + 2] == std::get<2>(d));
            }
            if (min_common == 0) {
                if (max_occ == 0) n_unmasked = want.size();
                else if (max_occ == 20) CHECK(want.size() < n_unmasked);
                else CHECK(want.size() == n_unmasked);
            }
        }
    }
    // an index without groups takes no query groups, and the reverse
    AnchorIndex plain(hdb, ndb, m, 1);
    std::vector<uint32_t> pairs, dist;
    CHECK(plain.match(hq, nq, {}, 1, 0, pairs, dist) > 0);
    try {
        plain.match(hq, nq, gq, 1, 0, pairs, dist);
        CHECK(!"groups against an index without groups were accepted");
    } catch (const KmuError &) {
    }
}

std::string random_read(uint64_t &state, size_t len) {
    std::string s(len, 'A');
    for (char &c : s) c = "ACGT"[next(state) & 3];
    return s;
}

void test_match_read_anchors_with_a_mask() {
    uint64_t state = 0xB10B;
    const std::string genome = random_read(state, 3000);
    std::vector<std::string> reads = {genome, genome.substr(0, 1500), genome.substr(500, 1500), random_read(state, 700)};
    std::vector<Sequence> seqs;
    for (const std::string &r : reads) seqs.emplace_back(std::string_view(r));
    const AnchorsGeneratorParameters params("reads.fasta", 500, 16, 21, 250);
    const auto anchors = gen_read_anchors<Kmer64bit>(params, 0, detail::pointers(seqs));
    const auto plain = match_read_anchors<Kmer64bit>(anchors, params, 4, 1);
    CHECK(!plain.empty());
    CHECK(match_read_anchors<Kmer64bit>(anchors, params, 4, 1, 1000) == plain);  // no key has 1000 slices
    const auto masked = match_read_anchors<Kmer64bit>(anchors, params, 4, 1, 1);  // only keys of a single slice seed: none pairs
    CHECK(masked.empty());
    CHECK(read_overlaps<Kmer64bit>(anchors, params, 4, 1, 1, 1, 2, 1000) == read_overlaps<Kmer64bit>(anchors, params, 4, 1, 1, 1, 2));
}

}  // namespace

int main() {
    int failed = 0;
    const std::pair<const char *, void (*)()> tests[] = {{"test_anchor_index", test_anchor_index},
                                                         {"test_match_read_anchors_with_a_mask", test_match_read_anchors_with_a_mask}};
    for (const auto &t : tests) {
        try {
            t.second();
            std::printf("ok %s\n", t.first);
        } catch (const std::exception &e) {
            std::printf("FAIL %s: %s\n", t.first, e.what());
            failed = 1;
        }
    }
    return failed;
}

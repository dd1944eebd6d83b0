// test_components -- components, components_knn and read_clusters of the C++ mirror (include/kmerutils.hpp) against answers
// computed here by a plain union-find: two components, an isolated node and skipped edges (records with a weight, then the
// neighbour lists of the same graph), one path of 5000 nodes given shuffled, and the clusters of reads cut from three genomes
// against the components of read_overlaps' own records.  Without a device it stops with the library's error ("no CPU fallback").
#include <algorithm>
#include <cstdio>
#include <numeric>
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

// the rules of include/kmu.h: the smaller root stays, clusters in the order of their smallest node, members by (cluster, node)
Components union_find(uint32_t n, const std::vector<std::pair<uint32_t, uint32_t>> &edges) {
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    auto find = [&](uint32_t x) {
        while (parent[x] != x) x = parent[x] = parent[parent[x]];
        return x;
    };
    for (const auto &e : edges) {
        if (e.first == e.second || e.first >= n || e.second >= n) continue;
        const uint32_t a = find(e.first), b = find(e.second);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
    }
    Components c;
    c.label.resize(n);
    c.cluster.resize(n);
    std::vector<uint32_t> rank(n, 0);
    for (uint32_t v = 0; v < n; v++) {
        c.label[v] = find(v);
        if (c.label[v] == v) {
            rank[v] = c.n_components++;
            c.size.push_back(0);
        }
    }
    for (uint32_t v = 0; v < n; v++) c.size[c.cluster[v] = rank[c.label[v]]]++;
    c.members.resize(n);
    std::iota(c.members.begin(), c.members.end(), 0u);
    std::stable_sort(c.members.begin(), c.members.end(), [&](uint32_t a, uint32_t b) { return c.cluster[a] < c.cluster[b]; });
    return c;
}

bool same(const Components &a, const Components &b) {
    return a.n_components == b.n_components && a.label == b.label && a.cluster == b.cluster && a.size == b.size && a.members == b.members;
}

std::string random_read(uint64_t &state, size_t len) {
    std::string s(len, 'A');
    for (char &c : s) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        c = "ACGT"[(state >> 33) & 3];
    }
    return s;
}

// {1, 4, 5} and {0, 3, 6}, 2 alone; 0 - 3 has weight 4; a self loop, a duplicate, both directions, ends out of range
void test_two_components_and_an_isolated_node() {
    const uint32_t n = 7;
    const std::vector<uint32_t> rec = {5, 1, 9, 2, 2, 9, 6, 3, 9, 4, 5, 9, 5, 4, 9, 3, 0, 4, 2, 7, 9, 0xFFFFFFFFu, 1, 9, 1, 5, 9};
    std::vector<std::pair<uint32_t, uint32_t>> all, heavy;
    for (size_t e = 0; e < rec.size(); e += 3) {
        all.push_back({rec[e], rec[e + 1]});
        if (rec[e + 2] >= 5) heavy.push_back({rec[e], rec[e + 1]});
    }
    const Components want = union_find(n, all);
    CHECK(want.n_components == 3 && want.size == (std::vector<uint32_t>{3, 3, 1}));
    CHECK(want.members == (std::vector<uint32_t>{0, 3, 6, 1, 4, 5, 2}));
    CHECK(same(components(rec, n, 3), want));
    CHECK(same(components(rec, n, 3, 2, 4), want));             // 0 - 3 counts at its own weight
    CHECK(same(components(rec, n, 3, 2, 5), union_find(n, heavy))); // ... and not above it: 0 is alone
    CHECK(union_find(n, heavy).n_components == 4);
    // the same graph as neighbour lists of 2 entries
    const uint32_t none = KMU_KNN_NONE;
    const std::vector<uint32_t> idx = {3, none, 5, 4, none, none, 6, 0, 5, 1, 4, none, 3, none};
    const std::vector<uint16_t> eq = {4, 0, 9, 9, 0, 0, 9, 4, 9, 9, 9, 0, 9, 0};
    CHECK(same(components_knn(idx, eq, n, 2, 4), want));
    CHECK(same(components_knn(idx, {}, n, 2), want));
    CHECK(same(components_knn(idx, eq, n, 2, 5), union_find(n, heavy)));
    CHECK(components_knn(idx, eq, n, 2, 10).n_components == n);
    CHECK(components(std::vector<uint32_t>{}, 4).size == (std::vector<uint32_t>{1, 1, 1, 1}));
    CHECK(components(std::vector<uint32_t>{}, 0).label.empty());
    bool thrown = false;
    try {
        components(std::vector<uint32_t>{0, 1, 2}, 4, 2);
    } catch (const std::invalid_argument &) {
        thrown = true;
    }
    CHECK(thrown);
    thrown = false;
    try {
        components_knn(idx, eq, n, 3);
    } catch (const std::invalid_argument &) {
        thrown = true;
    }
    CHECK(thrown);
}

void test_one_path_shuffled() {
    const uint32_t n = 5000;
    std::vector<uint32_t> at(n - 1);
    std::iota(at.begin(), at.end(), 0u);
    uint64_t state = 0xC0;
    for (size_t i = at.size() - 1; i > 0; i--) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        std::swap(at[i], at[(state >> 33) % (i + 1)]);
    }
    std::vector<uint32_t> edges;
    std::vector<std::pair<uint32_t, uint32_t>> list;
    for (uint32_t a : at) {
        edges.insert(edges.end(), {a + 1, a});
        list.push_back({a + 1, a});
    }
    const Components got = components(edges, n);
    CHECK(same(got, union_find(n, list)));
    CHECK(got.n_components == 1 && got.size[0] == n && *std::max_element(got.label.begin(), got.label.end()) == 0);
}

void test_read_clusters() {
    const uint32_t window = 200, overlap = 100, nbkmer = 16, first = 7;
    uint64_t state = 0x0E12;
    std::vector<std::string> reads;
    for (int mol = 0; mol < 3; mol++) {
        const std::string genome = random_read(state, 2800);
        for (int j = 0; j < 5; j++) reads.push_back(genome.substr(400 * j, 1200));
    }
    reads.push_back(random_read(state, 900));
    // the reads of a molecule are not neighbours in the batch: read i of the batch is read (7 i) mod 16 of the list above
    std::vector<Sequence> seqs;
    std::vector<int> molecule;
    for (size_t i = 0; i < reads.size(); i++) {
        const size_t src = (7 * i) % reads.size();
        seqs.emplace_back(std::string_view(reads[src]));
        molecule.push_back(src == 15 ? 3 : int(src / 5));
    }
    const AnchorsGeneratorParameters params("reads.fasta", window, nbkmer, 21, overlap);
    const auto anchors = gen_read_anchors<Kmer64bit>(params, first, detail::pointers(seqs), FHash::canon_value);
    for (bool by_votes : {false, true}) {
        const uint32_t min_score = by_votes ? 4 : 8;
        std::vector<std::pair<uint32_t, uint32_t>> edges;
        for (const Overlap &o : read_overlaps<Kmer64bit>(anchors, params, 2, 1, 2, 1, by_votes ? 0 : min_score))
            if (!by_votes || o.votes >= min_score) edges.push_back({o.readnum_a - first, o.readnum_b - first});
        const Components want = union_find(uint32_t(seqs.size()), edges);
        const ReadClusters got = read_clusters<Kmer64bit>(anchors, params, 2, 1, 2, 1, min_score, 0, by_votes);
        CHECK(got.cluster == want.cluster && got.size == want.size && got.members.size() == want.members.size());
        for (size_t i = 0; i < want.members.size(); i++) CHECK(got.members[i] == want.members[i] + first);
        // the clusters are the molecules
        std::vector<uint32_t> sizes = got.size;
        std::sort(sizes.begin(), sizes.end());
        CHECK(sizes == (std::vector<uint32_t>{1, 5, 5, 5}));
        for (size_t i = 0; i < seqs.size(); i++)
            for (size_t j = 0; j < seqs.size(); j++) CHECK((got.cluster[i] == got.cluster[j]) == (molecule[i] == molecule[j]));
    }
}

}  // namespace

int main() {
    try {
        test_two_components_and_an_isolated_node();
        test_one_path_shuffled();
        test_read_clusters();
        std::printf("ok test_components\n");
        return 0;
    } catch (const std::exception &e) {
        std::printf("FAIL test_components: %s\n", e.what());
        return 1;
    }
}

// sim_unitigs.cpp -- the functions of kmerutils_amd/csrc/kmu_ut_core.h, which the kernels of kmu_unitigs.hip are made of, over
// simulated lanes on random inputs, against straight replays: g++ only, no device, no libkmu.
//   layouts   random forests of paths and cycles (paths of 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129 and 1025 reads among them) with
//             shuffled read ids and strands, given as unique arcs with their mates in shuffled order, non-unique arcs mixed in: the
//             steps of the kernels in their order -- links, mates, init, the doubling rounds from one buffer into the other, the
//             cut, init and the rounds again, tails, the two scans, write -- against a sequential walk of the contract
//   faults    one fault planted in such a layout: the simulated checks must refuse it
//   copies    k_ut_seq_copy -- the tile walk of sim_gather.h with ut_src_index and ut_complement per byte -- against a byte loop per
//             step, with contributions of 0 and tiles that end inside, at and after an item
// usage: sim_unitigs [cases]; prints "ok sim_unitigs <checked items>" and exits 0, or the first mismatch and exits 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_ut_core.h"
#include "sim_gather.h"

using namespace kmu;

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}
static uint32_t below(uint32_t n) { return n ? (uint32_t) (rnd() % n) : 0u; }

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            printf("MISMATCH %s: ", #cond);       \
            printf(__VA_ARGS__);                  \
            printf("\n");                         \
            exit(1);                              \
        }                                         \
    } while (0)

static uint64_t g_checked = 0;

struct Layout {
    uint32_t n_reads = 0;
    std::vector<uint64_t> off;
    std::vector<kmu_sg_arc> arcs;
    std::vector<kmu_sg_read> reads;
};

struct Result {
    bool refused = false;
    std::vector<kmu_sg_unitig> unitigs;
    std::vector<kmu_sg_step> path;
    std::vector<kmu_sg_place> place;
};

static kmu_sg_arc arc(uint32_t from, uint32_t to, uint32_t len, uint32_t unique) { return kmu_sg_arc{from, to, len, 0u, 0u, 0u, unique, 0u}; }

// components of the given sizes (cycle[i]: component i is a circle; a circle has at least 2 reads), some contained reads and some
// arcs that are not unique
static Layout make_layout(const std::vector<uint32_t> &sizes, const std::vector<bool> &cycle, uint32_t n_contained) {
    Layout l;
    for (uint32_t s : sizes) l.n_reads += s;
    l.n_reads += n_contained;
    std::vector<uint32_t> ids(l.n_reads);
    for (uint32_t i = 0; i < l.n_reads; i++) ids[i] = i;
    for (uint32_t i = l.n_reads; i > 1; i--) std::swap(ids[i - 1], ids[below(i)]);
    std::vector<uint64_t> len(l.n_reads);
    for (auto &x : len) x = 500u + below(100);
    l.off.assign(l.n_reads + 1, 0);
    for (uint32_t r = 0; r < l.n_reads; r++) l.off[r + 1] = l.off[r] + len[r];
    l.reads.assign(l.n_reads, kmu_sg_read{0u, 0u, 0u, 0u});
    uint32_t at = 0;
    for (size_t c = 0; c < sizes.size(); c++) {
        std::vector<uint32_t> vs(sizes[c]);
        for (auto &v : vs) v = 2u * ids[at++] + below(2);
        const size_t n_arcs = cycle[c] ? vs.size() : vs.size() - 1;
        for (size_t i = 0; i < n_arcs; i++) {
            const uint32_t v = vs[i], w = vs[(i + 1) % vs.size()], ln = below(8) == 0 ? 0u : 150u + below(100);
            const uint64_t ovl = len[w >> 1] - ln; // the mate is as long as what v has to the left of the overlap
            l.arcs.push_back(arc(v, w, ln, 1u));
            l.arcs.push_back(arc(w ^ 1u, v ^ 1u, ovl < len[v >> 1] ? (uint32_t) (len[v >> 1] - ovl) : 0u, 1u));
        }
    }
    for (uint32_t i = 0; i < n_contained; i++) l.reads[ids[at++]].flags = KMU_SG_READ_CONTAINED;
    for (uint32_t i = 0; i < l.n_reads / 4; i++) { // arcs that do not count, hostile fields included
        kmu_sg_arc x = arc(below(4 * l.n_reads), below(4 * l.n_reads), below(2000), below(2) ? 0u : 2u);
        x.flags = below(2);
        l.arcs.push_back(x);
    }
    for (size_t i = l.arcs.size(); i > 1; i--) std::swap(l.arcs[i - 1], l.arcs[below((uint32_t) i)]);
    return l;
}

// the contract, walked
static Result walk(const Layout &l) {
    Result res;
    const uint32_t n_v = 2u * l.n_reads, NONE = KMU_SG_NONE;
    std::vector<uint32_t> next(n_v, NONE), prev(n_v, NONE), in(n_v, 0u);
    auto len = [&](uint32_t r) { return l.off[r + 1] - l.off[r]; };
    auto contained = [&](uint32_t r) { return (l.reads[r].flags & KMU_SG_READ_CONTAINED) != 0; };
    for (const auto &x : l.arcs) {
        if (x.unique != 1u) continue;
        if (x.from >= n_v || x.to >= n_v || (x.from >> 1) == (x.to >> 1) || x.len > len(x.to >> 1) || (x.flags & KMU_SG_ARC_REDUCED) ||
            contained(x.from >> 1) || contained(x.to >> 1) || next[x.from] != NONE || prev[x.to] != NONE) {
            res.refused = true;
            return res;
        }
        next[x.from] = x.to;
        prev[x.to] = x.from;
        in[x.to] = x.len;
    }
    for (uint32_t v = 0; v < n_v; v++)
        if (next[v] != NONE && next[next[v] ^ 1u] != (v ^ 1u)) {
            res.refused = true;
            return res;
        }
    struct Found {
        uint32_t min_v;
        std::vector<uint32_t> vs;
        bool cycle;
    };
    std::vector<Found> found;
    std::vector<bool> seen(n_v, false);
    for (int pass = 0; pass < 2; pass++)
        for (uint32_t v = 0; v < n_v; v++) {
            if (seen[v] || contained(v >> 1) || (pass == 0 && prev[v] != NONE)) continue;
            Found f{v, {v}, pass == 1};
            seen[v] = true;
            for (uint32_t w = next[v]; w != NONE && w != v; w = next[w]) {
                f.vs.push_back(w);
                seen[w] = true;
                f.min_v = std::min(f.min_v, w);
            }
            found.push_back(f);
        }
    std::vector<const Found *> kept;
    for (const auto &f : found)
        if (!(f.min_v & 1u)) kept.push_back(&f);
    std::sort(kept.begin(), kept.end(), [](const Found *a, const Found *b) { return a->min_v < b->min_v; });
    res.place.assign(l.n_reads, kmu_sg_place{0u, 0u, 0u, 0u});
    for (uint32_t r = 0; r < l.n_reads; r++)
        if (contained(r)) res.place[r].unitig = NONE;
    for (size_t u = 0; u < kept.size(); u++) {
        const Found &f = *kept[u];
        uint64_t end = 0;
        const uint64_t first = res.path.size();
        for (size_t i = 0; i < f.vs.size(); i++) {
            const uint32_t v = f.vs[i];
            end += (prev[v] != NONE) ? in[v] : len(v >> 1); // (the start of a cycle, the smallest vertex met first, has a prev)
            res.path.push_back(kmu_sg_step{v >> 1, v & 1u, end});
            res.place[v >> 1] = kmu_sg_place{(uint32_t) u, (uint32_t) i, v & 1u, 0u};
        }
        res.unitigs.push_back(kmu_sg_unitig{first, end, (uint32_t) f.vs.size(), f.cycle ? KMU_SG_UNITIG_CIRCULAR : 0u, f.min_v >> 1, 0u});
    }
    return res;
}

// the kernels of kmu_sg_unitigs, one loop iteration per lane, in launch order
static Result simulate(const Layout &l) {
    Result res;
    const uint32_t n_v = 2u * l.n_reads, NONE = KMU_SG_NONE;
    std::vector<uint32_t> next(n_v, NONE), prev(n_v, NONE), in(n_v, 0xDEADBEEFu), outdeg(n_v, 0u), indeg(n_v, 0u), pmin(n_v, NONE);
    std::vector<uint32_t> keep(l.n_reads, 0u), size(l.n_reads, 0u);
    auto len = [&](uint32_t r) { return l.off[r + 1] - l.off[r]; };
    auto contained = [&](uint32_t r) { return (l.reads[r].flags & KMU_SG_READ_CONTAINED) != 0; };
    bool bad = false;
    for (const auto &x : l.arcs) { // k_ut_links
        if (x.unique != 1u) continue;
        bool ok = ut_arc_range_ok(x, l.n_reads);
        if (ok) ok = ut_arc_reads_ok(x, len(x.to >> 1), l.reads[x.from >> 1].flags, l.reads[x.to >> 1].flags);
        if (ok) {
            const uint32_t o = outdeg[x.from]++, n = indeg[x.to]++;
            ok = o == 0u && n == 0u;
            if (o == 0u) next[x.from] = x.to;
            if (n == 0u) {
                prev[x.to] = x.from;
                in[x.to] = x.len;
            }
        }
        bad |= !ok;
    }
    for (uint32_t v = 0; v < n_v; v++) bad |= !ut_mate_ok(next.data(), v); // k_ut_mates
    std::vector<UtState> s[2] = {std::vector<UtState>(n_v), std::vector<UtState>(n_v)};
    std::vector<uint64_t> d[2] = {std::vector<uint64_t>(n_v), std::vector<uint64_t>(n_v)};
    const uint32_t rounds = ut_rounds(n_v);
    int cur = 0;
    bool cut = false;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && !cut) break; // (the kernels of the second pass return at once; both passes end in the same buffer)
        cur = 0;
        for (uint32_t v = 0; v < n_v; v++) { // k_ut_init
            s[0][v] = ut_state_init(v, prev[v]);
            d[0][v] = ut_contribution(indeg[v], in[v], len(v >> 1));
        }
        for (uint32_t r = 0; r < rounds; r++, cur ^= 1) // k_ut_round
            for (uint32_t v = 0; v < n_v; v++) s[cur ^ 1][v] = ut_round(s[cur].data(), d[cur].data(), v, d[cur ^ 1][v]);
        if (pass == 0)
            for (uint32_t v = 0; v < n_v; v++) { // k_ut_cut
                if (!ut_cycle_start(s[cur][v], v)) continue;
                const uint32_t p = prev[v];
                prev[v] = NONE;
                if (p < n_v) next[p] = NONE;
                cut = true;
            }
    }
    for (uint32_t v = 0; v < n_v; v++) { // k_ut_tails
        if (next[v] != NONE) continue;
        const UtState t = s[cur][v];
        CHECK(t.top < n_v && t.minv < n_v, "vertex %u", v);
        pmin[t.top] = t.minv;
        if (ut_kept(t.minv) && !contained(v >> 1)) {
            keep[t.minv >> 1] = 1u;
            size[t.minv >> 1] = t.cnt;
        }
    }
    std::vector<uint64_t> uid(l.n_reads + 1, 0), firsts(l.n_reads + 1, 0); // the scans
    for (uint32_t r = 0; r < l.n_reads; r++) {
        uid[r + 1] = uid[r] + keep[r];
        firsts[r + 1] = firsts[r] + size[r];
    }
    res.refused = bad;
    if (bad) return res; // (k_ut_write returns at once)
    CHECK(uid[l.n_reads] <= l.n_reads && firsts[l.n_reads] <= l.n_reads, "%llu unitigs", (unsigned long long) uid[l.n_reads]);
    res.unitigs.assign(uid[l.n_reads], kmu_sg_unitig{});
    res.path.assign(firsts[l.n_reads], kmu_sg_step{});
    res.place.assign(l.n_reads, kmu_sg_place{7u, 7u, 7u, 7u});
    std::vector<uint32_t> written(l.n_reads, 0u);
    for (uint32_t v = 0; v < n_v; v++) { // k_ut_write
        const uint32_t r = v >> 1, strand = v & 1u;
        if (contained(r)) {
            if (!strand) res.place[r] = kmu_sg_place{NONE, 0u, 0u, 0u};
            continue;
        }
        const UtState t = s[cur][v];
        CHECK(t.anc == NONE, "vertex %u still has an ancestor after the cut", v);
        const uint32_t m = pmin[t.top];
        CHECK(m < n_v, "the head %u of vertex %u got nothing published", t.top, v);
        if (!ut_kept(m)) continue;
        const uint32_t mr = m >> 1, rank = t.cnt - 1u;
        const uint64_t u = uid[mr], at = firsts[mr] + rank;
        CHECK(u < res.unitigs.size() && at < res.path.size(), "vertex %u", v);
        res.path[at] = kmu_sg_step{r, strand, d[cur][v]};
        res.place[r] = kmu_sg_place{(uint32_t) u, rank, strand, 0u};
        written[r]++;
        if (next[v] == NONE) {
            const bool circular = indeg[t.top] == 1u && prev[t.top] == NONE;
            res.unitigs[u] = kmu_sg_unitig{firsts[mr], d[cur][v], t.cnt, circular ? KMU_SG_UNITIG_CIRCULAR : 0u, mr, 0u};
        }
    }
    for (uint32_t r = 0; r < l.n_reads; r++) CHECK(written[r] == (contained(r) ? 0u : 1u), "read %u placed %u times", r, written[r]);
    return res;
}

static void compare(const Layout &l, const char *what) {
    const Result want = walk(l), got = simulate(l);
    CHECK(want.refused == got.refused, "%s: refusal %d against %d", what, (int) got.refused, (int) want.refused);
    if (want.refused) {
        g_checked++;
        return;
    }
    CHECK(want.unitigs.size() == got.unitigs.size() && want.path.size() == got.path.size(), "%s: %zu unitigs against %zu", what,
          got.unitigs.size(), want.unitigs.size());
    for (size_t u = 0; u < want.unitigs.size(); u++) {
        const auto &a = want.unitigs[u], &b = got.unitigs[u];
        CHECK(a.first == b.first && a.len == b.len && a.n_reads == b.n_reads && a.flags == b.flags && a.min_read == b.min_read && b.zero == 0u,
              "%s: unitig %zu: len %llu against %llu, %u reads against %u", what, u, (unsigned long long) b.len, (unsigned long long) a.len,
              b.n_reads, a.n_reads);
    }
    for (size_t i = 0; i < want.path.size(); i++)
        CHECK(want.path[i].read == got.path[i].read && want.path[i].strand == got.path[i].strand && want.path[i].end == got.path[i].end,
              "%s: step %zu", what, i);
    for (uint32_t r = 0; r < l.n_reads; r++) {
        const auto &a = want.place[r], &b = got.place[r];
        CHECK(a.unitig == b.unitig && a.rank == b.rank && a.strand == b.strand && b.zero == 0u, "%s: place of read %u", what, r);
    }
    g_checked += want.unitigs.size() + want.path.size() + l.n_reads;
}

static void layouts(uint32_t cases) {
    const uint32_t edges[] = {1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1025};
    for (uint32_t e : edges) { // one path alone (the round count sits at its edge), then one circle alone
        compare(make_layout({e}, {false}, 0), "one path");
        if (e >= 2) compare(make_layout({e}, {true}, 0), "one circle");
    }
    {
        std::vector<uint32_t> sizes(std::begin(edges), std::end(edges));
        std::vector<bool> cyc(sizes.size(), false);
        compare(make_layout(sizes, cyc, 5), "all edges as paths");
        for (size_t i = 1; i < cyc.size(); i++) cyc[i] = true;
        compare(make_layout(sizes, cyc, 5), "all edges as circles");
    }
    for (uint32_t c = 0; c < cases; c++) {
        std::vector<uint32_t> sizes;
        std::vector<bool> cyc;
        const uint32_t n = 1 + below(12);
        for (uint32_t i = 0; i < n; i++) {
            const bool circle = below(3) == 0;
            sizes.push_back((circle ? 2u : 1u) + below(below(4) == 0 ? 140u : 9u));
            cyc.push_back(circle);
        }
        compare(make_layout(sizes, cyc, below(4)), "random forest");
    }
}

static void faults(uint32_t cases) {
    for (uint32_t c = 0; c < cases; c++) {
        Layout l = make_layout({3u + below(6), 2u + below(6), 1u, 4u}, {false, true, false, false}, 2);
        std::vector<size_t> uniq;
        for (size_t i = 0; i < l.arcs.size(); i++)
            if (l.arcs[i].unique == 1u) uniq.push_back(i);
        kmu_sg_arc &x = l.arcs[uniq[below((uint32_t) uniq.size())]];
        uint32_t some_contained = 0;
        while (!(l.reads[some_contained].flags & KMU_SG_READ_CONTAINED)) some_contained++;
        switch (c % 8) {
        case 0: x.from = 2u * l.n_reads + below(5); break;
        case 1: x.to = 2u * l.n_reads + below(5); break;
        case 2: x.to = x.from ^ below(2); break;
        case 3: x.len = (uint32_t) (l.off[(x.to >> 1) + 1] - l.off[x.to >> 1]) + 1u + below(3); break;
        case 4: x.flags = KMU_SG_ARC_REDUCED; break;
        case 5: x.unique = 0u; break; // its mate has lost its mate
        case 6: x.to = 2u * some_contained; break;
        case 7: l.arcs.push_back(x); break; // twice: two out-arcs and two in-arcs
        }
        const Result want = walk(l), got = simulate(l);
        CHECK(want.refused && got.refused, "fault %u: refusal %d against %d", c % 8, (int) got.refused, (int) want.refused);
        g_checked++;
    }
}

// ---- the tile walk of k_ut_seq_copy ----------------------------------------------------------------------------------------------------
static void copies(uint32_t cases) {
    for (uint32_t c = 0; c < cases; c++) {
        // reads and a step list whose contributions are often 0 and sometimes long; one unitig after another
        const uint32_t n_reads = 1 + below(20);
        std::vector<uint64_t> off(n_reads + 1, 0);
        for (uint32_t r = 0; r < n_reads; r++) off[r + 1] = off[r] + 1u + below(below(3) == 0 ? 9000u : 300u);
        std::vector<uint8_t> bases(off[n_reads]);
        for (auto &b : bases) b = (uint8_t) "ACGTacgtNn-"[below(11)];
        const uint64_t target = c % 3 == 0 ? GATHER_TILE - 1u + (c / 3) % 3 : 0u; // totals at the tile size minus 1, at it and plus 1
        const uint64_t n_items = target ? 400 + below(100) : 1 + below(300);
        std::vector<kmu_sg_step> steps(n_items);
        std::vector<uint64_t> ends(n_items + 1, 0);
        std::vector<uint8_t> want;
        for (uint64_t j = 0; j < n_items; j++) {
            const uint32_t r = below(n_reads), strand = below(2);
            const uint64_t len = off[r + 1] - off[r];
            uint64_t cnt = below(3) == 0 ? 0u : 1u + below((uint32_t) len);
            if (target && ends[j] + cnt > target) cnt = target - ends[j]; // (then 0 for all that follow)
            steps[j] = kmu_sg_step{r, strand, ends[j] + cnt};
            ends[j + 1] = ends[j] + cnt;
            for (uint64_t k = 0; k < cnt; k++) { // the byte loop: the last cnt bytes of the read in the step's orientation
                const uint64_t pos = len - cnt + k; // in the oriented read
                want.push_back(strand ? ut_complement(bases[off[r] + (len - 1u - pos)]) : bases[off[r] + pos]);
            }
        }
        const uint64_t total = ends[n_items];
        std::vector<uint8_t> got(total, 0xEE);
        gather_replay(ends, [](const char *what) { CHECK(false, "%s", what); }, [&](uint64_t r, uint64_t o) {
            const kmu_sg_step s = steps[r];
            const uint64_t len = off[s.read + 1] - off[s.read];
            const uint64_t idx = ut_src_index(s.strand, len, ends[r + 1] - ends[r], o - ends[r]);
            CHECK(idx < len, "byte %llu", (unsigned long long) o);
            const uint8_t b = bases[off[s.read] + idx];
            got[o] = s.strand ? ut_complement(b) : b;
        });
        for (uint64_t o = 0; o < total; o++)
            CHECK(got[o] == want[o], "case %u byte %llu of %llu: %u against %u", c, (unsigned long long) o, (unsigned long long) total, got[o],
                  want[o]);
        g_checked += total;
    }
}

int main(int argc, char **argv) {
    const uint32_t cases = argc > 1 ? (uint32_t) atoi(argv[1]) : 200u;
    CHECK(ut_rounds(1) == 1 && ut_rounds(2) == 1 && ut_rounds(3) == 2 && ut_rounds(4) == 2 && ut_rounds(5) == 3 && ut_rounds(1ull << 32) == 32,
          "ut_rounds");
    layouts(cases);
    faults(cases);
    copies(cases);
    printf("ok sim_unitigs %llu\n", (unsigned long long) g_checked);
    return 0;
}

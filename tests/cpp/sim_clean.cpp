// sim_clean.cpp -- the functions of kmerutils_amd/csrc/kmu_clean_core.h, which the kernels of kmu_clean.hip are made of, over
// simulated lanes on random inputs, against a sequential restatement of the contract: g++ only, no device, no libkmu.
//   graphs   random planted graphs -- backbones with dead ends that enter or leave them and alternative paths around stretches of
//            them (tips of 63, 64 and 65 reads at T = 64 and branches of 64 and 65 reads at B = 64 among them), shuffled read ids and
//            strands, arcs with their mates in (from, to, rec) order, flagged arcs with hostile fields mixed in: the steps of the
//            kernels in launch order -- check, tips, spare, tipkill, flag, bubbles, flag, unique, reads -- with the lanes once in
//            ascending and once in descending order (the result may not depend on it), against walks of the contract
//   faults   one fault planted in such a graph: the simulated check must refuse it, as the restatement does
// usage: sim_clean [cases]; prints "ok sim_clean <checked items>" and exits 0, or the first mismatch and exits 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_clean_core.h"

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

static uint64_t g_checked = 0, g_removed[5] = {0, 0, 0, 0, 0}; // and the tips, tip reads, spared junctions, bubbles, bubble reads seen

struct Graph {
    uint32_t n_reads = 0;
    std::vector<kmu_sg_arc> arcs;
    std::vector<kmu_sg_read> reads;
    bool with_reads = false;
};
struct Result {
    bool refused = false;
    std::vector<kmu_sg_arc> arcs;
    std::vector<kmu_sg_read> reads;
    uint64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // in the order of kmu_sg_clean_stats
};
enum { TIPS, TIP_READS, SPARED, BUBBLES, BUBBLE_READS, ARCS_TIP, ARCS_BUBBLE, ARCS_LEFT };

static bool arc_less(const kmu_sg_arc &a, const kmu_sg_arc &b) { return std::tie(a.from, a.to, a.rec) < std::tie(b.from, b.to, b.rec); }

struct Plant {
    uint32_t n, where, m; // a tip of n reads at backbone[where] (m: 0 enters, 1 leaves), or a bubble of n reads around m from `where`
    bool bubble;
};
// one backbone per entry of `backs`, each with its plants; junk: flagged arcs with hostile fields mixed in
static Graph make_graph(const std::vector<uint32_t> &backs, const std::vector<std::vector<Plant>> &plants, bool junk, bool with_reads) {
    Graph g;
    std::vector<std::pair<uint32_t, uint32_t>> edges; // between logical nodes
    uint32_t n_nodes = 0;
    for (size_t c = 0; c < backs.size(); c++) {
        const uint32_t b0 = n_nodes;
        n_nodes += backs[c];
        for (uint32_t i = 0; i + 1 < backs[c]; i++) edges.push_back({b0 + i, b0 + i + 1});
        for (const Plant &p : plants[c]) {
            const uint32_t first = n_nodes;
            n_nodes += p.n;
            for (uint32_t i = 0; i + 1 < p.n; i++) edges.push_back({first + i, first + i + 1});
            if (p.bubble) {
                edges.push_back({b0 + p.where, first});
                edges.push_back({first + p.n - 1, b0 + p.where + p.m + 1});
            } else if (p.m) {
                edges.push_back({b0 + p.where, first});
            } else {
                edges.push_back({first + p.n - 1, b0 + p.where});
            }
        }
    }
    g.n_reads = n_nodes + 3; // (three reads without arcs)
    std::vector<uint32_t> ids(g.n_reads), flip(g.n_reads);
    for (uint32_t i = 0; i < g.n_reads; i++) ids[i] = i, flip[i] = below(2);
    for (uint32_t i = g.n_reads; i > 1; i--) std::swap(ids[i - 1], ids[below(i)]);
    for (size_t e = 0; e < edges.size(); e++) {
        const uint32_t v = 2u * ids[edges[e].first] + flip[edges[e].first], w = 2u * ids[edges[e].second] + flip[edges[e].second];
        g.arcs.push_back(kmu_sg_arc{v, w, 150u + below(100), 300u, (uint32_t) e, 0u, below(2), 0u});
        g.arcs.push_back(kmu_sg_arc{w ^ 1u, v ^ 1u, 150u + below(100), 300u, (uint32_t) e, 0u, below(2), 0u});
    }
    if (junk)
        for (uint32_t i = 0; i < g.n_reads / 3; i++) // arcs that do not survive: only `from` is in order with the rest
            g.arcs.push_back(kmu_sg_arc{below(2u * g.n_reads), below(8u * g.n_reads), below(2000), 0u, below(50), 1u + below(7), below(3), 0u});
    std::sort(g.arcs.begin(), g.arcs.end(), arc_less);
    g.with_reads = with_reads;
    g.reads.assign(g.n_reads, kmu_sg_read{0u, 0u, 0u, 0u});
    if (with_reads) {
        for (auto &r : g.reads) r = kmu_sg_read{0u, below(9), below(5), below(5)};
        g.reads[ids[n_nodes]].flags = KMU_SG_READ_CONTAINED; // (a read without arcs)
    }
    return g;
}

// ---- the contract, walked -------------------------------------------------------------------------------------------------------------
static Result walk(const Graph &g, uint32_t T, uint32_t B) {
    Result res;
    const uint32_t n_v = 2u * g.n_reads;
    const size_t n = g.arcs.size();
    for (size_t i = 1; i < n; i++)
        if (g.arcs[i].from < g.arcs[i - 1].from) res.refused = true;
    std::vector<bool> alive(n);
    std::set<std::tuple<uint32_t, uint32_t, uint32_t>> keys;
    for (size_t i = 0; i < n; i++) {
        const kmu_sg_arc &x = g.arcs[i];
        alive[i] = x.flags == 0u;
        if (!alive[i]) continue;
        if (x.from >= n_v || x.to >= n_v || (x.from >> 1) == (x.to >> 1)) {
            res.refused = true;
            continue;
        }
        if (g.with_reads && ((g.reads[x.from >> 1].flags | g.reads[x.to >> 1].flags) & KMU_SG_READ_CONTAINED)) res.refused = true;
        keys.insert({x.from, x.to, x.rec});
    }
    for (const auto &k : keys)
        if (!keys.count({std::get<1>(k) ^ 1u, std::get<0>(k) ^ 1u, std::get<2>(k)})) res.refused = true;
    if (res.refused) return res;
    std::vector<uint32_t> new_arc(n, 0u), new_read(g.n_reads, 0u);
    std::map<uint32_t, std::vector<uint32_t>> out;
    auto lists = [&]() {
        out.clear();
        for (size_t i = 0; i < n; i++)
            if (alive[i]) out[g.arcs[i].from].push_back(g.arcs[i].to);
    };
    auto deg = [&](uint32_t v) { return out.count(v) ? (uint32_t) out[v].size() : 0u; };
    auto remove = [&](const std::set<uint32_t> &gone, uint32_t bit, int stat) {
        for (uint32_t r : gone) new_read[r] |= bit;
        for (size_t i = 0; i < n; i++)
            if (alive[i] && (gone.count(g.arcs[i].from >> 1) || gone.count(g.arcs[i].to >> 1))) {
                alive[i] = false;
                new_arc[i] = bit;
                res.stats[stat]++;
            }
    };
    if (T) {
        lists();
        std::map<uint32_t, std::vector<uint32_t>> ends;
        for (uint32_t v0 = 0; v0 < n_v; v0++) {
            if (deg(v0 ^ 1u) != 0u || deg(v0) != 1u) continue;
            std::vector<uint32_t> w{v0};
            for (;;) {
                const uint32_t x = out[w.back()][0];
                if (deg(x ^ 1u) >= 2u) {
                    if (w.size() <= T) ends[w.back()] = w;
                    break;
                }
                if (deg(x) == 1u && w.size() < T) w.push_back(x);
                else break;
            }
        }
        std::set<uint32_t> spared, gone;
        for (uint32_t w = 0; w < n_v; w++) {
            if (deg(w ^ 1u) < 2u) continue;
            bool all = true;
            uint32_t best = KMU_SG_NONE;
            for (uint32_t x : out[w ^ 1u]) {
                const uint32_t u = x ^ 1u;
                if (!ends.count(u)) {
                    all = false;
                    break;
                }
                if (best == KMU_SG_NONE || ends[u].size() > ends[best].size() || (ends[u].size() == ends[best].size() && u < best)) best = u;
            }
            if (all) spared.insert(best), res.stats[SPARED]++;
        }
        for (const auto &e : ends)
            if (!spared.count(e.first)) {
                res.stats[TIPS]++;
                res.stats[TIP_READS] += e.second.size();
                for (uint32_t v : e.second) gone.insert(v >> 1);
            }
        remove(gone, KMU_SG_ARC_TIP, ARCS_TIP);
    }
    if (B) {
        lists();
        auto branch = [&](uint32_t a1, std::vector<uint32_t> &inner, uint32_t &t) {
            uint32_t x = a1;
            inner.clear();
            while (inner.size() < B) {
                if (deg(x ^ 1u) != 1u || deg(x) != 1u) return false;
                inner.push_back(x >> 1);
                x = out[x][0];
                if (deg(x ^ 1u) == 2u) {
                    t = x;
                    return true;
                }
            }
            return false;
        };
        std::set<uint32_t> gone;
        for (uint32_t s = 0; s < n_v; s++) {
            if (deg(s) != 2u) continue;
            std::vector<uint32_t> a, b;
            uint32_t ta = 0, tb = 0;
            if (!branch(out[s][0], a, ta) || !branch(out[s][1], b, tb) || ta != tb || (ta >> 1) == (s >> 1)) continue;
            const bool a_loses = a.size() != b.size() ? a.size() < b.size() : *std::min_element(a.begin(), a.end()) > *std::min_element(b.begin(), b.end());
            const std::vector<uint32_t> &loser = a_loses ? a : b;
            gone.insert(loser.begin(), loser.end());
            if (s < (ta ^ 1u)) res.stats[BUBBLES]++, res.stats[BUBBLE_READS] += loser.size();
        }
        remove(gone, KMU_SG_ARC_BUBBLE, ARCS_BUBBLE);
    }
    lists();
    res.arcs = g.arcs;
    for (size_t i = 0; i < n; i++) {
        res.arcs[i].flags |= new_arc[i];
        res.arcs[i].unique = alive[i] && deg(g.arcs[i].from) == 1u && deg(g.arcs[i].to ^ 1u) == 1u;
        res.stats[ARCS_LEFT] += alive[i];
    }
    res.reads = g.reads;
    for (uint32_t r = 0; r < g.n_reads; r++) {
        res.reads[r].flags |= new_read[r];
        res.reads[r].out_fwd = deg(2u * r);
        res.reads[r].out_rev = deg(2u * r + 1u);
    }
    return res;
}

// ---- the kernels, lane by lane --------------------------------------------------------------------------------------------------------
// lanes 0 .. n - 1 in ascending or descending order
template <class F> static void lanes(uint64_t n, bool descending, F f) {
    for (uint64_t i = 0; i < n; i++) f(descending ? n - 1u - i : i);
}

static Result simulate(const Graph &g, uint32_t T, uint32_t B, bool desc) {
    Result res;
    const uint32_t n_v = 2u * g.n_reads;
    const uint64_t n = g.arcs.size();
    const kmu_sg_arc *arcs = g.arcs.data();
    std::vector<uint32_t> deg1(n_v, 0u), deg2(n_v, 0u), deg3(n_v, 0u), sole1(n_v, KMU_SG_NONE), sole2(n_v, KMU_SG_NONE), tipcnt(n_v, 0u),
        spared(n_v, 0u), rflag(g.n_reads, 0u);
    bool bad = false;
    lanes(n, desc, [&](uint64_t i) { // k_cl_check
        const kmu_sg_arc x = arcs[i];
        if (i && x.from < arcs[i - 1u].from) bad = true;
        if (!cl_survives(x)) return;
        bool ok = cl_arc_ok(x, g.n_reads);
        if (ok && g.with_reads) ok = !((g.reads[x.from >> 1].flags | g.reads[x.to >> 1].flags) & KMU_SG_READ_CONTAINED);
        if (ok) ok = cl_has_mate(arcs, n, x);
        if (ok) {
            deg1[x.from]++;
            sole1[x.from] = std::min(sole1[x.from], x.to);
        }
        bad |= !ok;
    });
    if (bad) {
        res.refused = true;
        return res;
    }
    if (T) {
        lanes(n_v, desc, [&](uint64_t v) { // k_cl_tips
            const ClTip t = cl_tip_walk(deg1.data(), sole1.data(), (uint32_t) v, T);
            if (t.cnt) {
                CHECK(tipcnt[t.last] == 0u, "two tips end at %u", t.last);
                tipcnt[t.last] = t.cnt;
            }
        });
        lanes(n_v, desc, [&](uint64_t w) { // k_cl_spare
            const uint32_t u = cl_spared(arcs, n, deg1.data(), tipcnt.data(), (uint32_t) w);
            if (u == KMU_SG_NONE) return;
            CHECK(spared[u] == 0u, "%u spared twice", u);
            spared[u] = 1u;
            res.stats[SPARED]++;
        });
        lanes(n_v, desc, [&](uint64_t v0) { // k_cl_tipkill
            const ClTip t = cl_tip_walk(deg1.data(), sole1.data(), (uint32_t) v0, T);
            if (!t.cnt || spared[t.last]) return;
            uint32_t v = (uint32_t) v0;
            for (uint32_t i = 0; i < t.cnt; i++, v = sole1[v]) rflag[v >> 1] |= KMU_SG_READ_TIP;
            res.stats[TIPS]++;
            res.stats[TIP_READS] += t.cnt;
        });
    }
    res.arcs.assign(n, kmu_sg_arc{});
    auto flag = [&](const kmu_sg_arc *src, uint32_t bit, std::vector<uint32_t> &deg, std::vector<uint32_t> *sole, int stat, int stat_left) {
        lanes(n, desc, [&](uint64_t i) { // k_cl_flag
            const kmu_sg_arc x = src[i];
            uint32_t flags = x.flags;
            if (cl_survives(x)) {
                flags = cl_arc_flag(rflag[x.from >> 1], rflag[x.to >> 1], bit);
                if (flags) {
                    res.stats[stat]++;
                } else {
                    if (stat_left >= 0) res.stats[stat_left]++;
                    deg[x.from]++;
                    if (sole) (*sole)[x.from] = std::min((*sole)[x.from], x.to);
                }
            }
            res.arcs[i] = kmu_sg_arc{x.from, x.to, x.len, x.ovl, x.rec, flags, 0u, x.zero};
        });
    };
    flag(arcs, KMU_SG_ARC_TIP, deg2, &sole2, ARCS_TIP, -1);
    if (B)
        lanes(n_v, desc, [&](uint64_t s) { // k_cl_bubbles
            const ClBubble b = cl_bubble(res.arcs.data(), n, deg2.data(), sole2.data(), (uint32_t) s, B);
            if (!b.k) return;
            uint32_t v = b.first;
            for (uint32_t i = 0; i < b.k; i++, v = sole2[v]) rflag[v >> 1] |= KMU_SG_READ_BUBBLE;
            CHECK(v == b.t, "the loser of %u ends at %u, not %u", (uint32_t) s, v, b.t);
            if (cl_bubble_counts((uint32_t) s, b.t)) res.stats[BUBBLES]++, res.stats[BUBBLE_READS] += b.k;
        });
    flag(res.arcs.data(), KMU_SG_ARC_BUBBLE, deg3, nullptr, ARCS_BUBBLE, ARCS_LEFT);
    lanes(n, desc, [&](uint64_t i) { // k_cl_unique
        if (cl_unique(res.arcs[i], deg3.data())) res.arcs[i].unique = 1u;
    });
    res.reads.assign(g.n_reads, kmu_sg_read{0u, 0u, 0u, 0u});
    lanes(g.n_reads, desc, [&](uint64_t r) { // k_cl_reads
        kmu_sg_read x = g.with_reads ? g.reads[r] : kmu_sg_read{0u, 0u, 0u, 0u};
        x.flags |= rflag[r];
        x.out_fwd = deg3[2u * r];
        x.out_rev = deg3[2u * r + 1u];
        res.reads[r] = x;
    });
    return res;
}

static void compare(const Graph &g, uint32_t T, uint32_t B, const char *what) {
    Graph in = g;
    if (!in.with_reads) in.reads.assign(in.n_reads, kmu_sg_read{0u, 0u, 0u, 0u});
    const Result want = walk(in, T, B);
    for (int desc = 0; desc < 2; desc++) {
        const Result got = simulate(in, T, B, desc != 0);
        CHECK(got.refused == want.refused, "%s T %u B %u: refused %d, want %d", what, T, B, (int) got.refused, (int) want.refused);
        g_checked++;
        if (want.refused) continue;
        CHECK(!memcmp(got.stats, want.stats, sizeof got.stats), "%s T %u B %u: stats %llu %llu %llu %llu %llu, want %llu %llu %llu %llu %llu", what,
              T, B, (unsigned long long) got.stats[0], (unsigned long long) got.stats[1], (unsigned long long) got.stats[2],
              (unsigned long long) got.stats[3], (unsigned long long) got.stats[4], (unsigned long long) want.stats[0],
              (unsigned long long) want.stats[1], (unsigned long long) want.stats[2], (unsigned long long) want.stats[3],
              (unsigned long long) want.stats[4]);
        for (size_t i = 0; i < want.arcs.size(); i++)
            CHECK(!memcmp(&got.arcs[i], &want.arcs[i], sizeof(kmu_sg_arc)), "%s T %u B %u: arc %zu flags %u unique %u, want %u %u", what, T, B, i,
                  got.arcs[i].flags, got.arcs[i].unique, want.arcs[i].flags, want.arcs[i].unique);
        for (uint32_t r = 0; r < in.n_reads; r++)
            CHECK(!memcmp(&got.reads[r], &want.reads[r], sizeof(kmu_sg_read)), "%s T %u B %u: read %u flags %u, want %u", what, T, B, r,
                  got.reads[r].flags, want.reads[r].flags);
        g_checked += want.arcs.size() + in.n_reads + 8;
        for (int k = 0; k < 5; k++) g_removed[k] += want.stats[k];
    }
}

static Graph random_graph(bool junk, bool with_reads) {
    std::vector<uint32_t> backs;
    std::vector<std::vector<Plant>> plants;
    const uint32_t n_back = 1u + below(4);
    for (uint32_t c = 0; c < n_back; c++) {
        const uint32_t len = 30u + below(60);
        backs.push_back(len);
        std::vector<Plant> ps;
        uint32_t at = below(4);
        while (at + 12u < len) { // plants at increasing positions, sometimes at the same or the next one
            if (below(3) == 0u) {
                const uint32_t m = 1u + below(8);
                ps.push_back(Plant{1u + below(10), at, m, true});
                at += below(3) ? m + 1u + below(4) : m + 1u;
            } else {
                ps.push_back(Plant{1u + below(7), at, below(2), false});
                at += below(5);
            }
        }
        plants.push_back(ps);
    }
    return make_graph(backs, plants, junk, with_reads);
}

static const uint32_t LIMITS[][2] = {{4, 8}, {1, 1}, {0, 8}, {4, 0}, {64, 64}, {2, 3}, {7, 64}};

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    // the walk limits: tips of 63, 64 and 65 reads at T = 64 (entering and leaving), branches of 64 and 65 at B = 64
    for (uint32_t n : {63u, 64u, 65u})
        for (uint32_t leaves = 0; leaves < 2; leaves++) {
            const Graph g = make_graph({200u}, {{Plant{n, 100u, leaves, false}}}, false, false);
            compare(g, 64u, 0u, "long tip");
            compare(g, 64u, 64u, "long tip");
        }
    for (uint32_t k : {64u, 65u})
        for (uint32_t m : {1u, 64u, 65u}) {
            const Graph g = make_graph({100u}, {{Plant{k, 10u, m, true}}}, false, false);
            compare(g, 0u, 64u, "long branch");
            compare(g, 64u, 64u, "long branch");
        }
    for (int c = 0; c < cases; c++) {
        const Graph g = random_graph(c % 2 == 1, c % 3 == 2);
        for (const auto &l : LIMITS) compare(g, l[0], l[1], "random");
        // the output of a call is the input of the next
        Graph again = g;
        if (!again.with_reads) again.reads.assign(again.n_reads, kmu_sg_read{0u, 0u, 0u, 0u});
        const Result first = walk(again, 4u, 8u);
        CHECK(!first.refused, "a planted graph is refused");
        again.arcs = first.arcs;
        again.reads = first.reads;
        if (again.with_reads) compare(again, 4u, 8u, "second round"); // (removed reads keep their flags: TIP and BUBBLE are not CONTAINED)
        else compare(again, 64u, 64u, "second round");
        // every planted fault
        for (int fault = 0; fault < 6; fault++) {
            Graph bad = g;
            std::vector<size_t> live;
            for (size_t i = 0; i < bad.arcs.size(); i++)
                if (bad.arcs[i].flags == 0u) live.push_back(i);
            const size_t i = live[below((uint32_t) live.size())];
            kmu_sg_arc &x = bad.arcs[i];
            if (fault == 0) { // `from` decreases
                size_t j = i;
                while (j + 1 < bad.arcs.size() && bad.arcs[j + 1].from == x.from) j++;
                if (j + 1 >= bad.arcs.size()) continue;
                std::swap(bad.arcs[i], bad.arcs[j + 1]);
            } else if (fault == 1) {
                x.to = 2u * bad.n_reads + below(5);
            } else if (fault == 2) {
                x.to = x.from ^ 1u;
            } else if (fault == 3) { // no mate: the arc goes, its mate stays (everything after it keeps its order)
                bad.arcs.erase(bad.arcs.begin() + (long) i);
            } else if (fault == 4) {
                x.rec ^= 0x40000000u;
            } else {
                bad.with_reads = true;
                bad.reads[x.to >> 1].flags |= KMU_SG_READ_CONTAINED;
            }
            const Result want = walk(bad, 4u, 8u);
            CHECK(want.refused, "fault %d is not refused by the restatement", fault);
            compare(bad, 4u, 8u, "fault");
        }
    }
    for (int k = 0; k < 5; k++) CHECK(g_removed[k] >= (uint64_t) cases, "the cases removed too little: count %d is %llu", k, (unsigned long long) g_removed[k]);
    printf("ok sim_clean (%llu tips, %llu spared, %llu bubbles) %llu\n", (unsigned long long) g_removed[0], (unsigned long long) g_removed[2],
           (unsigned long long) g_removed[3], (unsigned long long) g_checked);
    return 0;
}

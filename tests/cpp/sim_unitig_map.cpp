// sim_unitig_map.cpp -- the functions of kmerutils_amd/csrc/kmu_um_core.h, which the kernels of kmu_unitig_map.hip are made of, over
// simulated lanes on random inputs, against a sequential restatement of the contract: g++ only, no device, no libkmu.
//   layouts  random forests of paths and cycles (unitigs of 1 .. 70 reads, shuffled read ids, both strands, cycles whose first steps
//            end before their reads' lengths, late reads longer than everything before them) with planted containments: records of
//            class A_CONTAINED and B_CONTAINED on both strands whose container is placed, is itself contained or projects below 0,
//            ties in length, and records of other classes with hostile fields mixed in: the steps of the kernels in launch order --
//            check, cand, flag, scan, write -- with the lanes once in ascending and once in descending order (the result may not
//            depend on it), against the contract written out sequentially
//   faults   one fault planted in such a layout: the simulated kernels must refuse it, as the restatement does
// usage: sim_unitig_map [cases]; prints "ok sim_unitig_map <checked items>" and exits 0, or the first mismatch and exits 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_um_core.h"

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

static uint64_t g_checked = 0, g_seen[3] = {0, 0, 0}; // and the layout, contained and unplaced reads seen

struct Layout {
    std::vector<kmu_sg_unitig> unitigs;
    std::vector<kmu_sg_step> path;
    std::vector<kmu_sg_place> place;
    std::vector<kmu_chain> chains;
    std::vector<uint8_t> classes;
    std::vector<uint64_t> off;
    uint32_t n_reads() const { return (uint32_t) place.size(); }
};
struct Result {
    bool refused = false;
    std::vector<kmu_chain> out;
    uint64_t stats[3] = {0, 0, 0}; // n_layout, n_contained, n_unplaced
};

static Layout make_layout(uint32_t n_unitigs, uint32_t n_contained) {
    Layout g;
    std::vector<uint32_t> sizes;
    uint32_t n_placed = 0;
    for (uint32_t u = 0; u < n_unitigs; u++) {
        const uint32_t pick = below(8), n = pick == 0 ? 1u : pick == 1 ? 2u : pick == 2 ? 64u : pick == 3 ? 65u : 1u + below(70);
        sizes.push_back(n);
        n_placed += n;
    }
    const uint32_t n_reads = n_placed + n_contained;
    std::vector<uint32_t> ids(n_reads);
    for (uint32_t i = 0; i < n_reads; i++) ids[i] = i;
    for (uint32_t i = n_reads; i > 1; i--) std::swap(ids[i - 1], ids[below(i)]);
    std::vector<uint64_t> len(n_reads);
    for (auto &l : len) l = 200u + below(1000);
    g.place.assign(n_reads, kmu_sg_place{KMU_SG_NONE, 0u, 0u, 0u});
    uint32_t next = 0;
    for (uint32_t u = 0; u < n_unitigs; u++) {
        const bool circular = below(4) == 0;
        const uint64_t first = g.path.size();
        uint64_t end = 0;
        uint32_t min_read = KMU_SG_NONE;
        for (uint32_t rank = 0; rank < sizes[u]; rank++) {
            const uint32_t r = ids[next++], s = below(2);
            if (below(16) == 0) len[r] = 3000u + below(1000); // longer than everything before it, more often than not
            end += (rank == 0 && !circular) ? len[r] : 1u + below((uint32_t) len[r]);
            g.path.push_back(kmu_sg_step{r, s, end});
            g.place[r] = kmu_sg_place{u, rank, s, 0u};
            min_read = std::min(min_read, r);
        }
        g.unitigs.push_back(kmu_sg_unitig{first, end, sizes[u], circular ? KMU_SG_UNITIG_CIRCULAR : 0u, min_read, 0u});
    }
    g.off.assign(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) g.off[r + 1] = g.off[r] + len[r];
    // the records: for every contained read a few candidates, with ties in length; then junk of other classes
    auto segment = [&](uint32_t r, uint32_t want, uint32_t &s, uint32_t &e) {
        const uint32_t l = (uint32_t) len[r], n = std::min(want, l);
        s = below(l - n + 1);
        e = s + n;
    };
    for (uint32_t i = n_placed; i < n_reads && n_placed; i++) {
        const uint32_t c = ids[i], n_rec = below(5);
        const uint32_t tie = 50u + below(150);
        for (uint32_t k = 0; k < n_rec; k++) {
            const uint32_t g_read = below(6) == 0 ? ids[n_placed + below(n_contained)] : ids[below(n_placed)];
            if (g_read == c) continue;
            uint32_t cs, ce, gs, ge;
            segment(c, below(2) ? tie : 1u + below(200), cs, ce);
            segment(g_read, below(3) ? ce - cs : 1u + below(400), gs, ge);
            if (below(4) == 0) gs = 0, ge = std::min<uint32_t>(ge ? ge : 1u, (uint32_t) len[g_read]); // near the read's start: often below 0 on a cycle
            const uint32_t s = below(2);
            if (below(2)) {
                g.chains.push_back(kmu_chain{c, g_read, s, below(100), below(100), below(100), cs, ce, gs, ge});
                g.classes.push_back(KMU_SG_A_CONTAINED);
            } else {
                g.chains.push_back(kmu_chain{g_read, c, s, below(100), below(100), below(100), gs, ge, cs, ce});
                g.classes.push_back(KMU_SG_B_CONTAINED);
            }
        }
        if (below(3) == 0) { // other classes are not looked at, whatever they hold
            const uint32_t cls[5] = {KMU_SG_SKIP, KMU_SG_SHORT, KMU_SG_LOWID, KMU_SG_INTERNAL, KMU_SG_DOVETAIL};
            g.chains.push_back(kmu_chain{below(2) ? c : n_reads + below(9), below(2) ? ids[below(n_placed)] : 0xFFFFFFFFu, below(4), 0u, 0u, 0u,
                                         below(5000), below(5000), below(5000), below(5000)});
            g.classes.push_back((uint8_t) cls[below(5)]);
        }
    }
    for (size_t i = g.chains.size(); i > 1; i--) { // records in any order
        const size_t j = below((uint32_t) i);
        std::swap(g.chains[i - 1], g.chains[j]);
        std::swap(g.classes[i - 1], g.classes[j]);
    }
    return g;
}

// ---- the kernels of kmu_unitig_map.hip, lane by lane ------------------------------------------------------------------------------
template <class F> static void lanes(uint64_t n, bool descending, F f) {
    for (uint64_t i = 0; i < n; i++) f(descending ? n - 1 - i : i);
}

static Result simulate(const Layout &g, bool descending) {
    Result res;
    const uint32_t n_reads = g.n_reads();
    const uint64_t n_unitigs = g.unitigs.size(), n_steps = g.path.size(), n_chains = g.chains.size();
    uint32_t bad = 0;
    std::vector<unsigned long long> best(n_reads, 0ull);
    std::vector<uint32_t> has(n_reads, 0u);
    std::vector<kmu_chain> out(n_reads, kmu_chain{7u, 7u, 7u, 7u, 7u, 7u, 7u, 7u, 7u, 7u});
    auto length = [&](uint32_t r) { return g.off[r + 1u] - g.off[r]; };
    // k_um_check
    lanes(n_unitigs, descending, [&](uint64_t u) { bad |= !um_unitig_ok(g.unitigs[u], n_steps); });
    lanes(n_steps, descending, [&](uint64_t i) { bad |= !um_step_ok(g.path[i], n_reads); });
    lanes(n_reads, descending, [&](uint64_t r) { bad |= !um_place_ok(g.unitigs.data(), n_unitigs, g.path.data(), n_steps, g.place[r], (uint32_t) r); });
    // k_um_cand
    if (!bad) lanes(n_chains, descending, [&](uint64_t x) {
        const uint32_t cls = g.classes[x];
        if (!um_is_containment(cls)) return;
        const kmu_chain rec = g.chains[x];
        if (!um_rec_reads_ok(rec, n_reads) || !um_rec_segs_ok(rec, length(rec.read_a), length(rec.read_b))) {
            bad = 1u;
            return;
        }
        const UmCand k = um_cand(rec, cls);
        if (g.place[k.c].unitig != KMU_SG_NONE) return;
        const kmu_sg_place pg = g.place[k.g];
        if (pg.unitig == KMU_SG_NONE) return;
        const uint64_t e_g = g.path[g.unitigs[pg.unitig].first + pg.rank].end;
        if (um_project(k, pg.strand, e_g, length(k.g)) < 0) return;
        best[k.c] = std::max(best[k.c], um_key(k, x)); // atomicMax
    });
    if (bad) {
        res.refused = true;
        return res;
    }
    // k_um_flag, the scan, k_um_write
    lanes(n_reads, descending, [&](uint64_t r) {
        const bool layout = g.place[r].unitig != KMU_SG_NONE, contained = !layout && best[r] != 0ull;
        has[r] = layout || contained;
        res.stats[0] += layout;
        res.stats[1] += contained;
    });
    std::vector<uint64_t> pos(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) pos[r + 1] = pos[r] + has[r];
    lanes(n_reads, descending, [&](uint64_t r) {
        if (!has[r]) return;
        const kmu_sg_place p = g.place[r];
        if (p.unitig != KMU_SG_NONE) {
            out[pos[r]] = um_layout_record(p.unitig, (uint32_t) r, p.strand, g.path[g.unitigs[p.unitig].first + p.rank].end, length((uint32_t) r));
        } else {
            const uint32_t x = um_key_index(best[r]);
            const kmu_chain rec = g.chains[x];
            const UmCand k = um_cand(rec, g.classes[x]);
            const kmu_sg_place pg = g.place[k.g];
            const uint64_t e_g = g.path[g.unitigs[pg.unitig].first + pg.rank].end;
            out[pos[r]] = um_contained_record(k, x, rec.strand, pg.unitig, pg.strand, um_project(k, pg.strand, e_g, length(k.g)));
        }
    });
    res.stats[2] = n_reads - res.stats[0] - res.stats[1];
    out.resize(pos[n_reads]);
    res.out = out;
    return res;
}

// ---- the contract, sequentially ---------------------------------------------------------------------------------------------------
static Result restate(const Layout &g) {
    Result res;
    const int64_t n_reads = g.n_reads(), n_steps = (int64_t) g.path.size(), n_unitigs = (int64_t) g.unitigs.size();
    auto length = [&](int64_t r) { return (int64_t) (g.off[r + 1] - g.off[r]); };
    res.refused = true;
    for (const auto &u : g.unitigs)
        if (u.first > (uint64_t) n_steps || u.first + u.n_reads > (uint64_t) n_steps || u.len >> 32) return res;
    for (const auto &s : g.path)
        if (s.read >= n_reads || s.strand > 1 || s.end == 0) return res;
    for (int64_t r = 0; r < n_reads; r++) {
        const auto &p = g.place[r];
        if (p.unitig == KMU_SG_NONE) continue;
        if (p.unitig >= n_unitigs || p.rank >= g.unitigs[p.unitig].n_reads) return res;
        const auto &s = g.path[g.unitigs[p.unitig].first + p.rank];
        if (s.read != r || s.strand != p.strand || s.end > g.unitigs[p.unitig].len) return res;
    }
    for (size_t x = 0; x < g.chains.size(); x++) {
        const auto &c = g.chains[x];
        if (g.classes[x] != KMU_SG_A_CONTAINED && g.classes[x] != KMU_SG_B_CONTAINED) continue;
        if (c.read_a >= n_reads || c.read_b >= n_reads || c.strand > 1 || c.a_start > c.a_end || c.b_start > c.b_end) return res;
        if (c.a_end > length(c.read_a) || c.b_end > length(c.read_b)) return res;
    }
    res.refused = false;
    for (int64_t r = 0; r < n_reads; r++) {
        const auto &p = g.place[r];
        if (p.unitig != KMU_SG_NONE) {
            const int64_t e = (int64_t) g.path[g.unitigs[p.unitig].first + p.rank].end, L = length(r), t = std::min(L, e);
            res.out.push_back(kmu_chain{p.unitig, (uint32_t) r, p.strand, 0u, KMU_SG_NONE, KMU_SG_NONE, (uint32_t) (e - t), (uint32_t) e,
                                        (uint32_t) (p.strand ? 0 : L - t), (uint32_t) (p.strand ? t : L)});
            res.stats[0]++;
            continue;
        }
        int64_t best_len = -1;
        kmu_chain best{};
        for (size_t x = 0; x < g.chains.size(); x++) { // ascending x: the first of the longest stays
            const auto &c = g.chains[x];
            int64_t container, cs, ce, gs, ge;
            if (g.classes[x] == KMU_SG_A_CONTAINED && c.read_a == r) container = c.read_b, cs = c.a_start, ce = c.a_end, gs = c.b_start, ge = c.b_end;
            else if (g.classes[x] == KMU_SG_B_CONTAINED && c.read_b == r) container = c.read_a, cs = c.b_start, ce = c.b_end, gs = c.a_start, ge = c.a_end;
            else continue;
            const auto &pg = g.place[container];
            if (pg.unitig == KMU_SG_NONE) continue;
            const int64_t e_g = (int64_t) g.path[g.unitigs[pg.unitig].first + pg.rank].end, L_g = length(container);
            const int64_t a_start = e_g - L_g + (pg.strand ? L_g - ge : gs);
            if (a_start < 0 || ce - cs <= best_len) continue;
            best_len = ce - cs;
            best = kmu_chain{pg.unitig, (uint32_t) r, pg.strand ^ c.strand, 1u, (uint32_t) x, (uint32_t) container, (uint32_t) a_start,
                             (uint32_t) (a_start + ge - gs), (uint32_t) cs, (uint32_t) ce};
        }
        if (best_len >= 0) {
            res.out.push_back(best);
            res.stats[1]++;
        } else {
            res.stats[2]++;
        }
    }
    return res;
}

static void compare(const Layout &g, const char *what) {
    const Result want = restate(g);
    for (int descending = 0; descending < 2; descending++) {
        const Result got = simulate(g, descending != 0);
        CHECK(got.refused == want.refused, "%s: refused %d, wanted %d", what, got.refused, want.refused);
        g_checked++;
        if (want.refused) continue;
        CHECK(got.out.size() == want.out.size(), "%s: %zu records, wanted %zu", what, got.out.size(), want.out.size());
        for (size_t i = 0; i < want.out.size(); i++) {
            CHECK(memcmp(&got.out[i], &want.out[i], sizeof(kmu_chain)) == 0, "%s: record %zu of read %u (score %u, a %u .. %u; wanted score %u, a %u .. %u)",
                  what, i, want.out[i].read_b, got.out[i].score, got.out[i].a_start, got.out[i].a_end, want.out[i].score, want.out[i].a_start,
                  want.out[i].a_end);
            CHECK(i == 0 || want.out[i - 1].read_b < want.out[i].read_b, "%s: read ids do not ascend at %zu", what, i);
            g_checked++;
        }
        for (int k = 0; k < 3; k++) {
            CHECK(got.stats[k] == want.stats[k], "%s: stat %d is %llu, wanted %llu", what, k, (unsigned long long) got.stats[k], (unsigned long long) want.stats[k]);
            if (!descending) g_seen[k] += want.stats[k];
        }
    }
}

static void faults(const Layout &good) {
    const uint32_t n_reads = good.n_reads();
    uint32_t placed = 0, rec = KMU_SG_NONE;
    while (good.place[placed].unitig == KMU_SG_NONE) placed++;
    for (size_t x = 0; x < good.chains.size() && rec == KMU_SG_NONE; x++)
        if (good.classes[x] == KMU_SG_A_CONTAINED || good.classes[x] == KMU_SG_B_CONTAINED) rec = (uint32_t) x;
    const kmu_sg_place p = good.place[placed];
    const uint64_t at = good.unitigs[p.unitig].first + p.rank;
    for (int f = 0; f < 18; f++) {
        Layout g = good;
        switch (f) {
        case 0: g.unitigs.back().first = g.path.size(); g.unitigs.back().n_reads = 1; break;
        case 1: g.unitigs[0].n_reads = (uint32_t) g.path.size() + 1u; break;
        case 2: g.unitigs[below((uint32_t) g.unitigs.size())].len = 1ull << 32; break;
        case 3: g.unitigs.back().first = ~0ull; break;
        case 4: g.path[below((uint32_t) g.path.size())].read = n_reads; break;
        case 5: g.path[below((uint32_t) g.path.size())].strand = 2; break;
        case 6: g.path[below((uint32_t) g.path.size())].end = 0; break;
        case 7: g.path[at].end = g.unitigs[p.unitig].len + 1; break;
        case 8: g.place[placed].unitig = (uint32_t) g.unitigs.size(); break;
        case 9: g.place[placed].rank = g.unitigs[p.unitig].n_reads; break;
        case 10: g.place[placed].strand ^= 1u; break;
        case 11: g.path[at].read = (g.path[at].read + 1u) % n_reads; break;
        case 12: if (rec == KMU_SG_NONE) continue; g.chains[rec].read_a = n_reads; break;
        case 13: if (rec == KMU_SG_NONE) continue; g.chains[rec].read_b = 0xFFFFFFFFu; break;
        case 14: if (rec == KMU_SG_NONE) continue; g.chains[rec].strand = 2; break;
        case 15: if (rec == KMU_SG_NONE) continue; g.chains[rec].a_start = g.chains[rec].a_end + 1; break;
        case 16: if (rec == KMU_SG_NONE) continue; g.chains[rec].b_end = (uint32_t) (g.off[g.chains[rec].read_b + 1] - g.off[g.chains[rec].read_b]) + 1; break;
        case 17: if (rec == KMU_SG_NONE) continue; g.chains[rec].a_end = (uint32_t) (g.off[g.chains[rec].read_a + 1] - g.off[g.chains[rec].read_a]) + 1; break;
        }
        CHECK(restate(g).refused, "fault %d is not refused by the restatement", f);
        compare(g, "fault");
    }
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 100;
    for (int c = 0; c < cases; c++) {
        const Layout g = make_layout(1u + below(12), below(60));
        compare(g, "layout");
        if (c % 4 == 0) faults(g);
    }
    {
        Layout g = make_layout(0, 5); // nothing is placed: every read is unplaced, whatever the records say
        compare(g, "no unitigs");
        Layout none;
        none.off.push_back(0);
        compare(none, "no reads");
    }
    CHECK(g_seen[0] && g_seen[1] && g_seen[2], "layout %llu, contained %llu, unplaced %llu reads: a branch was never taken",
          (unsigned long long) g_seen[0], (unsigned long long) g_seen[1], (unsigned long long) g_seen[2]);
    printf("ok sim_unitig_map %llu\n", (unsigned long long) g_checked);
    return 0;
}

// sim_string_graph.cpp -- the functions of kmerutils_amd/csrc/kmu_sg_core.h, which the kernels of kmu_string_graph.hip are made of,
// over 64 simulated lanes on random inputs, against straight replays: g++ only, no device, no libkmu.
//   records   random chain records of random reads: sg_record_ok / sg_lengths_ok against the list of faults, sg_class against a
//             replay of the contract in signed arithmetic, the contained flags, and the compaction of k_sg_arcs (tiles of KMU_SG_TILE,
//             chunks of 64 lanes, ballot and prefix count) with sg_arc_pair; the mates mirror each other
//   arc sets  the arcs of those records, and random arc sets over few vertices so that duplicate arcs, long runs, runs that start at
//             index 0 and runs that end at the last arc are common: sg_lower_from and sg_run_begin against linear scans,
//             sg_vertex_stats against a scan under (len, to, rec), and the reduction -- one simulated wave per arc f, its lanes
//             striding over out(to) through sg_reduce_step -- against a brute-force triple loop over all (f, g, h)
// usage: sim_string_graph [cases]; prints "ok sim_string_graph <checked items>" and exits 0, or the first mismatch and exits 1
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_sg_core.h"

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

// the contract's class, replayed in signed 64-bit arithmetic
static uint32_t replay_class(const kmu_chain &c, long long la, long long lb, const kmu_chain_aln *aln, const kmu_sg_params &p) {
    if (c.read_a >= c.read_b) return KMU_SG_SKIP;
    const long long oa = (long long) c.a_end - c.a_start, ob = (long long) c.b_end - c.b_start;
    if (oa < p.min_overlap || ob < p.min_overlap) return KMU_SG_SHORT;
    if (aln && (!(aln->flags & 1u) || (long long) aln->matches * 1000 < (long long) p.min_identity_permille * ((long long) aln->matches + aln->edit)))
        return KMU_SG_LOWID;
    const long long bs = c.strand ? lb - c.b_end : c.b_start, be = c.strand ? lb - c.b_start : c.b_end;
    const long long aL = c.a_start, aR = la - c.a_end, bL = bs, bR = lb - be;
    const long long hang = std::min(aL, bL) + std::min(aR, bR), maplen = std::max(oa, ob);
    if (hang > p.max_hang || hang * 1000 > maplen * p.int_permille) return KMU_SG_INTERNAL;
    const bool a_in = aL <= bL && aR <= bR, b_in = aL >= bL && aR >= bR;
    if (a_in && b_in) return la < lb ? KMU_SG_A_CONTAINED : KMU_SG_B_CONTAINED;
    return a_in ? KMU_SG_A_CONTAINED : b_in ? KMU_SG_B_CONTAINED : KMU_SG_DOVETAIL;
}

static bool arc_less(const kmu_sg_arc &x, const kmu_sg_arc &y) {
    if (x.from != y.from) return x.from < y.from;
    if (x.to != y.to) return x.to < y.to;
    return x.rec < y.rec;
}

// everything that is checked on a sorted arc list over n_v vertices; n_rec bounds the rec field
static void check_arc_set(const std::vector<kmu_sg_arc> &arcs, uint32_t n_v, uint32_t n_rec, uint32_t fuzz) {
    const uint64_t n = arcs.size();
    const kmu_sg_arc *A = arcs.data();
    // slices
    std::vector<uint64_t> off(n_v + 1);
    for (uint32_t v = 0; v <= n_v; v++) {
        uint64_t lin = 0;
        while (lin < n && A[lin].from < v) lin++;
        off[v] = sg_lower_from(A, n, v);
        CHECK(off[v] == lin, "sg_lower_from v %u: %llu, scan %llu", v, (unsigned long long) off[v], (unsigned long long) lin);
        g_checked++;
    }
    CHECK(off[n_v] == n, "the last offset");
    // L and first
    std::vector<uint32_t> max_len(n_v);
    std::vector<uint64_t> first(n_v);
    for (uint32_t v = 0; v < n_v; v++) {
        sg_vertex_stats(A, off[v], off[v + 1], max_len[v], first[v]);
        uint32_t m = 0;
        uint64_t best = off[v + 1];
        for (uint64_t i = off[v]; i < off[v + 1]; i++) {
            m = std::max(m, A[i].len);
            if (best == off[v + 1] || A[i].len < A[best].len || (A[i].len == A[best].len && arc_less(A[i], A[best]))) best = i;
        }
        CHECK(max_len[v] == m && first[v] == best, "sg_vertex_stats v %u", v);
        // run search: every x, present or not
        for (uint32_t x = 0; x <= n_v; x++) {
            uint64_t lin = off[v];
            while (lin < off[v + 1] && A[lin].to < x) lin++;
            CHECK(sg_run_begin(A, off[v], off[v + 1], x) == lin, "sg_run_begin v %u x %u", v, x);
            g_checked++;
        }
    }
    // the reduction: one simulated wave per arc, 64 lanes striding over out(w)
    std::vector<uint8_t> mark(n_rec, 0), brute(n_rec, 0);
    for (uint64_t f = 0; f < n; f++) {
        const uint32_t v = A[f].from, w = A[f].to;
        if (w >= n_v) continue;
        for (uint64_t j0 = off[w]; j0 < off[w + 1]; j0 += 64)
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint64_t j = j0 + lane;
                if (j < off[w + 1])
                    sg_reduce_step(A, A[f].len, off[v], off[v + 1], max_len[v], j, first[w], fuzz, [&](uint32_t rec) {
                        CHECK(rec < n_rec, "mark out of range");
                        mark[rec] = 1;
                    });
            }
    }
    for (uint64_t f = 0; f < n; f++)
        for (uint64_t g = 0; g < n; g++) {
            if (A[g].from != A[f].to) continue;
            const uint32_t v = A[f].from, w = A[f].to;
            uint64_t fw = n;
            for (uint64_t i = 0; i < n; i++)
                if (A[i].from == w && (fw == n || A[i].len < A[fw].len || (A[i].len == A[fw].len && arc_less(A[i], A[fw])))) fw = i;
            uint64_t lv = 0;
            for (uint64_t i = 0; i < n; i++)
                if (A[i].from == v) lv = std::max<uint64_t>(lv, A[i].len);
            if (!((uint64_t) A[f].len + A[g].len <= lv + fuzz || A[g].len < fuzz || g == fw)) continue;
            for (uint64_t h = 0; h < n; h++)
                if (A[h].from == v && A[h].to == A[g].to) brute[A[h].rec] = 1;
        }
    for (uint32_t r = 0; r < n_rec; r++) CHECK(mark[r] == brute[r], "mark of record %u: %u, brute force %u", r, mark[r], brute[r]);
    g_checked += n_rec + n;
}

static void case_records() {
    const uint32_t n_reads = 2 + below(30);
    std::vector<uint64_t> off(n_reads + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++) off[r + 1] = off[r] + (below(8) == 0 ? 0 : below(1500));
    kmu_sg_params p{below(120), below(4) == 0 ? 0xFFFFFFFFu : below(400), below(1001), below(1001), below(3) ? below(40) : 0u, 0u};
    const uint64_t n = below(3) == 0 ? KMU_SG_TILE * 2 + below(130) : below(400);
    std::vector<kmu_chain> chains(n);
    std::vector<kmu_chain_aln> aln(n);
    const bool with_aln = below(2);
    std::vector<uint8_t> cls(n);
    std::vector<uint32_t> contained(n_reads, 0);
    for (uint64_t c = 0; c < n; c++) {
        kmu_chain r{};
        r.read_a = below(n_reads);
        r.read_b = below(n_reads);
        r.strand = below(2);
        const uint32_t la = (uint32_t) (off[r.read_a + 1] - off[r.read_a]), lb = (uint32_t) (off[r.read_b + 1] - off[r.read_b]);
        // overlaps that mostly touch an end of each read, so that every class occurs
        const uint32_t oa = below(la + 1), ob = std::min(lb, below(3) ? oa + below(7) : below(lb + 1));
        r.a_start = below(2) ? la - oa : below(2) ? 0u : below(la - oa + 1);
        r.a_end = r.a_start + oa;
        r.b_start = below(2) ? lb - ob : below(2) ? 0u : below(lb - ob + 1);
        r.b_end = r.b_start + ob;
        bool faulty = false;
        switch (below(40)) { // a fault now and then
        case 0: r.read_a = n_reads + below(3); faulty = true; break;
        case 1: r.read_b = 0xFFFFFFFFu; faulty = true; break;
        case 2: r.strand = 2 + below(5); faulty = true; break;
        case 3: r.a_start = r.a_end + 1; faulty = true; break;
        case 4: r.b_end = lb + 1 + below(9); faulty = true; break;
        case 5: r.a_end = la + 1; faulty = true; break;
        default: break;
        }
        aln[c] = kmu_chain_aln{below(200), below(1000), 0u, below(8) ? 1u : 0u};
        chains[c] = r;
        bool ok = sg_record_ok(r, n_reads);
        if (ok) ok = sg_lengths_ok(r, off[r.read_a + 1] - off[r.read_a], off[r.read_b + 1] - off[r.read_b]);
        CHECK(ok == !faulty, "record %llu: ok %d, planted fault %d", (unsigned long long) c, ok, faulty);
        cls[c] = KMU_SG_SKIP;
        if (ok) {
            cls[c] = (uint8_t) sg_class(r, la, lb, with_aln ? &aln[c] : nullptr, p);
            const uint32_t want = replay_class(r, la, lb, with_aln ? &aln[c] : nullptr, p);
            CHECK(cls[c] == want, "class of record %llu: %u, replay %u", (unsigned long long) c, cls[c], want);
            if (cls[c] == KMU_SG_A_CONTAINED) contained[r.read_a] = 1;
            if (cls[c] == KMU_SG_B_CONTAINED) contained[r.read_b] = 1;
        }
        g_checked++;
    }
    // k_sg_arcs: COUNT per tile, the scan, WRITE
    const uint32_t n_tiles = (uint32_t) std::max<uint64_t>(1, (n + KMU_SG_TILE - 1) / KMU_SG_TILE);
    std::vector<uint64_t> coff(n_tiles + 1, 0);
    std::vector<kmu_sg_arc> arcs;
    for (int write = 0; write < 2; write++)
        for (uint32_t tile = 0; tile < n_tiles; tile++) {
            uint64_t at = write ? coff[tile] : 0;
            for (uint32_t c0 = 0; c0 < KMU_SG_TILE; c0 += 64) {
                uint64_t bal = 0;
                for (uint32_t lane = 0; lane < 64; lane++) {
                    const uint64_t c = (uint64_t) tile * KMU_SG_TILE + c0 + lane;
                    if (c < n && cls[c] == KMU_SG_DOVETAIL && !contained[chains[c].read_a] && !contained[chains[c].read_b]) bal |= 1ull << lane;
                }
                if (write)
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        if (!((bal >> lane) & 1ull)) continue;
                        const uint64_t c = (uint64_t) tile * KMU_SG_TILE + c0 + lane;
                        const uint64_t q = at + (uint64_t) __builtin_popcountll(bal & ((1ull << lane) - 1ull));
                        CHECK(2 * q + 1 < arcs.size(), "survivor %llu behind the total", (unsigned long long) q);
                        const kmu_chain &r = chains[c];
                        kmu_sg_arc x, y;
                        sg_arc_pair(r, off[r.read_a + 1] - off[r.read_a], off[r.read_b + 1] - off[r.read_b], (uint32_t) c, x, y);
                        CHECK(x.len >= 1 && y.len >= 1 && y.from == (x.to ^ 1u) && y.to == (x.from ^ 1u), "the arcs of record %llu are no mates",
                              (unsigned long long) c);
                        CHECK((x.from >> 1) == r.read_a && (y.from >> 1) == r.read_b && x.ovl == r.a_end - r.a_start && y.ovl == r.b_end - r.b_start,
                              "sides of record %llu", (unsigned long long) c);
                        // x.len: how far b reaches beyond a on the side a is left through, in signed arithmetic
                        const long long la = (long long) (off[r.read_a + 1] - off[r.read_a]), lb = (long long) (off[r.read_b + 1] - off[r.read_b]);
                        const long long bL = r.strand ? lb - r.b_end : r.b_start, bR = r.strand ? r.b_start : lb - r.b_end;
                        const long long aL = r.a_start, aR = la - r.a_end;
                        const bool right = !(x.from & 1u);
                        CHECK((long long) x.len == (right ? bR - aR : bL - aL) && (long long) y.len == (right ? aL - bL : aR - bR), "lengths of record %llu",
                              (unsigned long long) c);
                        arcs[2 * q] = x;
                        arcs[2 * q + 1] = y;
                    }
                at += (uint64_t) __builtin_popcountll(bal);
            }
            if (!write) coff[tile + 1] = coff[tile] + at;
            if (!write && tile + 1 == n_tiles) arcs.assign(2 * coff[n_tiles], kmu_sg_arc{});
        }
    for (size_t i = 2; i < arcs.size(); i += 2) CHECK(arcs[i - 2].rec < arcs[i].rec, "survivors out of record order");
    std::stable_sort(arcs.begin(), arcs.end(), [](const kmu_sg_arc &x, const kmu_sg_arc &y) { return sg_arc_key(x) < sg_arc_key(y); });
    for (size_t i = 1; i < arcs.size(); i++) CHECK(!arc_less(arcs[i], arcs[i - 1]), "a stable sort by key is not (from, to, rec) order");
    if (arcs.size() <= 240) check_arc_set(arcs, 2 * n_reads, (uint32_t) n, p.fuzz);
    g_checked += arcs.size();
}

static void case_arc_set() {
    const uint32_t n_v = 1 + below(9), n_rec = 1 + below(60), fuzz = below(3) ? below(30) : 0u;
    std::vector<kmu_sg_arc> arcs(below(5) == 0 ? 64 + below(140) : below(70));
    for (auto &a : arcs) a = kmu_sg_arc{below(n_v), below(n_v), 1 + below(below(2) ? 60 : 6), 0u, below(n_rec), 0u, 0u, 0u};
    std::sort(arcs.begin(), arcs.end(), arc_less);
    check_arc_set(arcs, n_v, n_rec, fuzz);
}

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    for (int i = 0; i < cases; i++) {
        case_records();
        case_arc_set();
        case_arc_set();
    }
    printf("ok sim_string_graph %llu\n", (unsigned long long) g_checked);
    return 0;
}

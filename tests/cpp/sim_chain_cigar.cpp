// sim_chain_cigar -- host only, no device and no libkmu: the functions of kmerutils_amd/csrc/kmu_align_core.h driven over 64
// simulated lanes exactly as k_cigar_sweep and k_cigar_walk drive them: the sweep of sim_chain_align.cpp with the direction bits of
// every pair-step ORed into a word per lane and stored to the chain's slab row by row, then the walk over blocks of ALIGN_WALK_ROWS
// staged rows with the runs written downwards from the end of the slab.  Compared with a backtrack over a full matrix of the same
// 64-bit keys by the value rule of include/kmu.h (diagonal, then up, then left).  Random, related and two-letter pairs, both
// strands' streams, every instance (C = 1, 2, 4, 8) that can take the chain's n_diags; directed lengths put the number of pair-steps
// at 1, 2 and one below, at and above multiples of 8 / C and of the walk's block; a short max_run checks how runs are cut.  Every
// slab and block access is bounds-checked.  tests/test_chain_cigar_sim.py builds and runs it; an argument sets the number of random
// cases.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include <algorithm>
#include "../../kmerutils_amd/csrc/kmu_align_core.h"
using namespace kmu;

static uint32_t code2b(uint32_t c) { uint32_t x = (c >> 1) & 3u; return x ^ (x >> 1); }
struct View { const std::string *base; uint64_t begin, len; };
static uint32_t code_word(const View &v, uint64_t widx) {
    uint64_t a0 = (v.begin & ~15ull) + 16 * widx;
    uint32_t w = 0;
    for (int i = 0; i < 16; i++) {
        char ch = a0 + i < v.base->size() ? (*v.base)[a0 + i] : 'A';
        w |= code2b((uint8_t) ch) << (30 - 2 * i);
    }
    return w;
}
static uint32_t stream_word(const View &v, const AlignStream &s, uint32_t strand, int32_t k) {
    if (k < 0 || (uint32_t) k >= s.n_words) return 0;
    uint32_t w = code_word(v, strand ? s.n_words - 1u - (uint32_t) k : (uint32_t) k);
    return strand ? ~w : align_rev16(w);
}
[[noreturn]] static void die(const char *what) { printf("FAIL %s\n", what); exit(1); }

// the sweep with TRACE: returns the key of (m, n); slab: the chain's rows, every word written exactly once
template <int C> uint64_t sim_sweep(const AlignGeom &g, const View &va, const View &vb, uint32_t strand, std::vector<uint32_t> &slab) {
    constexpr uint32_t S = 8 / C;
    const AlignStream sa = align_stream(va.begin & 15, g.m, 0), sb = align_stream(vb.begin & 15, g.n, strand);
    const uint64_t rows = align_trace_rows(g.steps, C);
    slab.assign(rows * 64, 0xDEADBEEFu);
    std::vector<uint8_t> written(rows * 64, 0);
    auto store = [&](uint64_t at, uint32_t w) {
        if (at >= slab.size()) die("trace store outside the slab");
        if (written[at]++) die("trace word stored twice");
        slab[at] = w;
    };
    uint64_t ve[64][C], vo[64][C];
    uint32_t i0[64], j0[64], acc[64];
    uint32_t win_a[ALIGN_WIN_WORDS], win_b[ALIGN_WIN_WORDS];
    for (int l = 0; l < 64; l++) {
        for (int c = 0; c < C; c++) ve[l][c] = vo[l][c] = ALN_INF;
        i0[l] = (uint32_t) g.I0 - C * l; j0[l] = (uint32_t) g.J0 + C * l; acc[l] = 0;
    }
    uint32_t pa[64], pb[64]; AlignWords na[64], nb[64]; uint64_t wa[64], wb[64];
    for (uint32_t u0 = 0, chunk = 0; u0 < g.steps; u0 += ALIGN_CHUNK, chunk++) {
        const int32_t fa = align_first_a<C>(sa, g, chunk), fb = align_first_b(sb, g, chunk);
        for (uint32_t k = 0; k < ALIGN_WIN_WORDS; k++) { win_a[k] = stream_word(va, sa, 0, fa + (int32_t) k); win_b[k] = stream_word(vb, sb, strand, fb + (int32_t) k); }
        const uint32_t uend = g.steps - u0 < ALIGN_CHUNK ? g.steps : u0 + ALIGN_CHUNK;
        for (uint32_t l = 0; l < 64; l++) {
            pa[l] = align_pos_a<C>(sa, g, fa, u0, l); pb[l] = align_pos_b<C>(sb, g, fb, u0, l);
            na[l] = align_read(win_a, pa[l]); nb[l] = align_read(win_b, pb[l]);
        }
        for (uint32_t ub = u0; ub < uend; ub += ALIGN_REFILL) {
            for (uint32_t l = 0; l < 64; l++) {
                wa[l] = align_window(na[l], pa[l]); wb[l] = align_window(nb[l], pb[l]);
                pa[l] += ALIGN_REFILL; pb[l] += ALIGN_REFILL;
                na[l] = align_read(win_a, pa[l]); nb[l] = align_read(win_b, pb[l]);
            }
            const uint32_t cnt = uend - ub < ALIGN_REFILL ? uend - ub : ALIGN_REFILL;
            for (uint32_t s = 0; s < cnt; s++) {
                uint64_t fl[64], fr[64];
                uint32_t bits[64];
                for (int l = 0; l < 64; l++) fl[l] = l ? vo[l - 1][C - 1] : ALN_INF;
                for (int l = 0; l < 64; l++) {
                    bits[l] = align_even_dirs<C>(ve[l], vo[l], fl[l], wa[l], wb[l]);
                    align_even<C>(ve[l], vo[l], fl[l], wa[l], wb[l], i0[l], j0[l], 2u * C * l, g);
                }
                for (int l = 0; l < 64; l++) fr[l] = l < 63 ? ve[l + 1][0] : ALN_INF;
                for (int l = 0; l < 64; l++) {
                    bits[l] |= align_odd_dirs<C>(ve[l], vo[l], fr[l], wa[l], wb[l]);
                    acc[l] |= bits[l] << (4u * C * (s % S));
                    if (s % S == S - 1u) { store((uint64_t) ((ub + s) / S) * 64u + l, acc[l]); acc[l] = 0; }
                    align_odd<C>(ve[l], vo[l], fr[l], wa[l], wb[l], i0[l], j0[l], 2u * C * l, g);
                    wa[l] >>= 2; wb[l] >>= 2; i0[l]++; j0[l]++;
                }
            }
            if (cnt % S) for (int l = 0; l < 64; l++) { store((uint64_t) ((ub + cnt - 1u) / S) * 64u + l, acc[l]); acc[l] = 0; }
        }
    }
    for (uint8_t w : written) if (w != 1) die("a trace word was never stored");
    const uint32_t kf = g.ef % (2u * C), lf = g.ef / (2u * C);
    return (kf & 1) ? vo[lf][kf >> 1] : ve[lf][kf >> 1];
}

// the walk as k_cigar_walk runs it; returns the runs in path order as they lie at the end of the slab
template <int C> std::vector<uint32_t> sim_walk(const AlignGeom &g, std::vector<uint32_t> &slab, uint32_t max_run) {
    const uint32_t rows = (uint32_t) (slab.size() / 64);
    std::vector<uint32_t> blk(ALIGN_WALK_ROWS * 64, 0);
    uint32_t blk_lo = rows, count = 0, last_row = rows;
    auto read = [&](const AlignSlot &s) -> uint32_t {
        if (s.row >= rows || s.lane >= 64 || s.shift > 30 || (s.shift & 1)) die("slot outside the slab");
        if (s.row > last_row) die("the walk moved to a later row");
        last_row = s.row;
        if (s.row < blk_lo) {
            blk_lo = align_walk_block(s.row);
            // what is staged now must not have been overwritten by runs: they occupy the last `count` words of the slab
            if ((uint64_t) (s.row + 1) * 64u > slab.size() - count) die("runs were written over rows not yet staged");
            for (uint32_t r = 0; r < ALIGN_WALK_ROWS && blk_lo + r <= s.row; r++)
                for (uint32_t l = 0; l < 64; l++) blk[r * 64u + l] = slab[(uint64_t) (blk_lo + r) * 64u + l];
        }
        if (s.row - blk_lo >= ALIGN_WALK_ROWS) die("row above the staged block");
        return (blk[(s.row - blk_lo) * 64u + s.lane] >> s.shift) & 3u;
    };
    auto emit = [&](uint32_t run) {
        count++;
        if (count > slab.size()) die("more runs than the slab holds");
        slab[slab.size() - count] = run;
    };
    align_walk<C>(g, read, emit, max_run);
    return std::vector<uint32_t>(slab.end() - count, slab.end());
}

static char comp(char c) { switch (c & 0xDF) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; default: return 'A'; } }

// full matrix, then the backtrack by values; returns the key of (m, n)
static uint64_t brute(const std::string &A, const std::string &B, int band, uint32_t max_run, std::vector<uint32_t> &runs) {
    int m = A.size(), n = B.size();
    int lo = std::min(0, n - m) - band, hi = std::max(0, n - m) + band;
    std::vector<std::vector<uint64_t>> D(m + 1, std::vector<uint64_t>(n + 1, ALN_INF));
    auto eq = [&](int i, int j) { return (A[i - 1] & 0xDF) == (B[j - 1] & 0xDF); };
    for (int i = 0; i <= m; i++) for (int j = 0; j <= n; j++) {
        if (j - i < lo || j - i > hi) continue;
        if (i == 0 && j == 0) { D[i][j] = 0xFFFFFFFFull; continue; }
        uint64_t v = ALN_INF;
        if (i > 0 && D[i - 1][j] != ALN_INF) v = std::min(v, D[i - 1][j] + ALN_EDIT);
        if (j > 0 && D[i][j - 1] != ALN_INF) v = std::min(v, D[i][j - 1] + ALN_EDIT);
        if (i > 0 && j > 0 && D[i - 1][j - 1] != ALN_INF) v = std::min(v, eq(i, j) ? D[i - 1][j - 1] - 1 : D[i - 1][j - 1] + ALN_EDIT);
        D[i][j] = v;
    }
    std::string path; // ops from (m, n) backwards
    for (int i = m, j = n; i || j;) {
        if (i == 0) { path += 'D'; j--; }
        else if (j == 0) { path += 'I'; i--; }
        else if (D[i - 1][j - 1] != ALN_INF && (eq(i, j) ? D[i - 1][j - 1] - 1 : D[i - 1][j - 1] + ALN_EDIT) == D[i][j]) { path += eq(i, j) ? '=' : 'X'; i--; j--; }
        else if (D[i - 1][j] != ALN_INF && D[i - 1][j] + ALN_EDIT == D[i][j]) { path += 'I'; i--; }
        else { if (D[i][j - 1] == ALN_INF || D[i][j - 1] + ALN_EDIT != D[i][j]) die("brute: no move explains the value"); path += 'D'; j--; }
    }
    std::reverse(path.begin(), path.end());
    runs.clear();
    for (size_t x = 0; x < path.size();) {
        size_t y = x;
        while (y < path.size() && path[y] == path[x]) y++;
        const uint32_t code = path[x] == '=' ? 7u : path[x] == 'X' ? 8u : path[x] == 'I' ? 1u : 2u;
        uint32_t len = (uint32_t) (y - x);
        if (len % max_run) runs.push_back(((len % max_run) << 4) | code); // the remainder first
        for (uint32_t k = 0; k < len / max_run; k++) runs.push_back((max_run << 4) | code);
        x = y;
    }
    return D[m][n];
}

static long checked = 0;
static void one_case(const std::string &all, int ba, int m, int bb, int n, uint32_t strand, uint32_t band, uint32_t max_run, const char *what) {
    const uint32_t nd = align_n_diags(m, n, band);
    if (nd > 1024) return;
    const AlignGeom g = align_geom(m, n, band);
    View va{&all, (uint64_t) ba, (uint64_t) m}, vb{&all, (uint64_t) bb, (uint64_t) n};
    std::string A = all.substr(ba, m), B = all.substr(bb, n);
    if (strand) { std::string R(n, 'A'); for (int x = 0; x < n; x++) R[x] = comp(B[n - 1 - x]); B = R; }
    std::vector<uint32_t> want, slab;
    const uint64_t want_key = brute(A, B, band, max_run, want);
    for (int C : {1, 2, 4, 8}) {
        if (nd > 128u * C) continue;
        const uint64_t key = C == 1 ? sim_sweep<1>(g, va, vb, strand, slab) : C == 2 ? sim_sweep<2>(g, va, vb, strand, slab) : C == 4 ? sim_sweep<4>(g, va, vb, strand, slab) : sim_sweep<8>(g, va, vb, strand, slab);
        const std::vector<uint32_t> got = C == 1 ? sim_walk<1>(g, slab, max_run) : C == 2 ? sim_walk<2>(g, slab, max_run) : C == 4 ? sim_walk<4>(g, slab, max_run) : sim_walk<8>(g, slab, max_run);
        checked++;
        if (key != want_key || got != want) {
            printf("MISMATCH %s C %d m %d n %d band %u strand %u steps %u max_run %u: %zu runs, want %zu\n", what, C, m, n, band, strand, g.steps, max_run, got.size(), want.size());
            for (size_t x = 0; x < std::min<size_t>(12, std::max(got.size(), want.size())); x++)
                printf("  run %zu: got %x want %x\n", x, x < got.size() ? got[x] : 0, x < want.size() ? want[x] : 0);
            exit(1);
        }
        if (max_run == ALIGN_MAX_RUN && got.size() > 2u * (uint32_t) (want_key >> 32) + 1u) die("more than 2 edit + 1 runs");
    }
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 600;
    srand(7);
    const char *alpha = "ACGTacgt";
    // the hand example that pins the tie rule: AA against A is 1I1=
    {
        std::string all = "AAA";
        std::vector<uint32_t> want;
        brute("AA", "A", 1, ALIGN_MAX_RUN, want);
        if (want != std::vector<uint32_t>{(1u << 4) | 1u, (1u << 4) | 7u}) die("AA / A is not 1I1=");
        one_case(all, 0, 2, 2, 1, 0, 1, ALIGN_MAX_RUN, "hand");
        one_case(all, 0, 1, 1, 2, 0, 1, ALIGN_MAX_RUN, "hand mirror");
    }
    // directed: m = n at an even band makes steps = m + 1
    const int targets[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025};
    for (int T : targets) for (int kind = 0; kind < 4; kind++) {
        const int m = T - 1, total = 2 * m + 40;
        std::string all(total, 'A');
        for (auto &c : all) c = alpha[rand() % (kind == 1 ? 2 : 8)];
        const uint32_t strand = kind & 1;
        const int ba = rand() % 17, bb = m + 17 + rand() % 17;
        if (kind >= 2) for (int x = 0; x < m; x++) if (rand() % 12) { char c = all[ba + x]; all[strand ? bb + m - 1 - x : bb + x] = strand ? comp(c) : c; }
        const uint32_t band = kind == 3 ? 64 : 2; // (band 64: C = 2 and above only)
        if (align_geom(m, m, band).steps != (uint32_t) T) die("directed case: steps");
        one_case(all, ba, m, bb, m, strand, band, ALIGN_MAX_RUN, "directed");
        one_case(all, ba, m, bb, m, strand, band, 3, "directed, short runs");
    }
    for (int rep = 0; rep < reps; rep++) {
        int total = 50 + rand() % 3000;
        std::string all(total, 'A');
        int nalpha = (rep % 3 == 0) ? 2 : 8;
        for (auto &c : all) c = alpha[rand() % nalpha];
        int maxlen = (rep % 10 == 0) ? 1400 : 90;
        int m = rand() % std::min(maxlen, total / 2), n;
        if (rand() % 2) n = std::max(0, std::min(total / 2 - 1, m + rand() % 41 - 20)); else n = rand() % std::min(maxlen, total / 2);
        int ba = rand() % (total / 2 - m + 1), bb = total / 2 + rand() % (total - total / 2 - n + 1);
        uint32_t strand = rand() & 1;
        if (rand() % 2) { // B similar to A
            for (int x = 0; x < n && x < m; x++) if (rand() % 10) { char c = all[ba + x]; all[strand ? bb + n - 1 - x : bb + x] = strand ? comp(c) : c; }
        }
        int bandmax = rep % 7 == 0 ? 511 : 40;
        uint32_t band = rand() % (bandmax + 1);
        one_case(all, ba, m, bb, n, strand, band, rep % 5 == 0 ? 1 + rand() % 6 : ALIGN_MAX_RUN, "random");
    }
    printf("ok sim_chain_cigar %ld\n", checked);
    return 0;
}

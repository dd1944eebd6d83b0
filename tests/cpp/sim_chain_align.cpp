// sim_chain_align -- host only, no device and no libkmu: the functions of kmerutils_amd/csrc/kmu_align_core.h driven over 64
// simulated lanes exactly as k_chain_align drives them (staging per chunk, window reads one refill ahead, the two neighbour values
// per pair-step), against a full-matrix banded DP over the same 64-bit keys.  Random segments at random places of a random batch,
// both strands, every instance (C = 1, 2, 4, 8) that can take the chain's n_diags; also checks that no window read leaves the staged
// words.  tests/test_chain_align_sim.py builds and runs it; an argument sets the number of cases.
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

template <int C> uint64_t sim_chain(const AlignGeom &g, const View &va, const View &vb, uint32_t strand) {
    const AlignStream sa = align_stream(va.begin & 15, g.m, 0), sb = align_stream(vb.begin & 15, g.n, strand);
    uint64_t ve[64][C], vo[64][C];
    uint32_t i0[64], j0[64];
    uint32_t win_a[ALIGN_WIN_WORDS], win_b[ALIGN_WIN_WORDS];
    for (int l = 0; l < 64; l++) {
        for (int c = 0; c < C; c++) ve[l][c] = vo[l][c] = ALN_INF;
        i0[l] = (uint32_t) g.I0 - C * l; j0[l] = (uint32_t) g.J0 + C * l;
    }
    uint32_t pa[64], pb[64]; AlignWords na[64], nb[64]; uint64_t wa[64], wb[64];
    for (uint32_t u0 = 0, chunk = 0; u0 < g.steps; u0 += ALIGN_CHUNK, chunk++) {
        const int32_t fa = align_first_a<C>(sa, g, chunk), fb = align_first_b(sb, g, chunk);
        for (uint32_t k = 0; k < ALIGN_WIN_WORDS; k++) { win_a[k] = stream_word(va, sa, 0, fa + (int32_t) k); win_b[k] = stream_word(vb, sb, strand, fb + (int32_t) k); }
        const uint32_t uend = g.steps - u0 < ALIGN_CHUNK ? g.steps : u0 + ALIGN_CHUNK;
        for (uint32_t l = 0; l < 64; l++) {
            pa[l] = align_pos_a<C>(sa, g, fa, u0, l); pb[l] = align_pos_b<C>(sb, g, fb, u0, l);
            if ((pa[l] >> 4) + 2 >= ALIGN_WIN_WORDS || (pb[l] >> 4) + 2 >= ALIGN_WIN_WORDS) { printf("window overflow\n"); exit(1); }
            na[l] = align_read(win_a, pa[l]); nb[l] = align_read(win_b, pb[l]);
        }
        for (uint32_t ub = u0; ub < uend; ub += ALIGN_REFILL) {
            for (uint32_t l = 0; l < 64; l++) {
                wa[l] = align_window(na[l], pa[l]); wb[l] = align_window(nb[l], pb[l]);
                pa[l] += ALIGN_REFILL; pb[l] += ALIGN_REFILL;
                if ((pa[l] >> 4) + 2 >= ALIGN_WIN_WORDS || (pb[l] >> 4) + 2 >= ALIGN_WIN_WORDS) { printf("window overflow 2\n"); exit(1); }
                na[l] = align_read(win_a, pa[l]); nb[l] = align_read(win_b, pb[l]);
            }
            const uint32_t cnt = uend - ub < ALIGN_REFILL ? uend - ub : ALIGN_REFILL;
            for (uint32_t s = 0; s < cnt; s++) {
                uint64_t fl[64], fr[64];
                for (int l = 0; l < 64; l++) fl[l] = l ? vo[l - 1][C - 1] : ALN_INF;
                for (int l = 0; l < 64; l++) align_even<C>(ve[l], vo[l], fl[l], wa[l], wb[l], i0[l], j0[l], 2u * C * l, g);
                for (int l = 0; l < 64; l++) fr[l] = l < 63 ? ve[l + 1][0] : ALN_INF;
                for (int l = 0; l < 64; l++) {
                    align_odd<C>(ve[l], vo[l], fr[l], wa[l], wb[l], i0[l], j0[l], 2u * C * l, g);
                    wa[l] >>= 2; wb[l] >>= 2; i0[l]++; j0[l]++;
                }
            }
        }
    }
    const uint32_t kf = g.ef % (2u * C), lf = g.ef / (2u * C);
    return (kf & 1) ? vo[lf][kf >> 1] : ve[lf][kf >> 1];
}

static char comp(char c) { switch (c & 0xDF) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; default: return 'A'; } }

static uint64_t brute(const std::string &A, const std::string &B, int band) {
    int m = A.size(), n = B.size();
    int lo = std::min(0, n - m) - band, hi = std::max(0, n - m) + band;
    std::vector<std::vector<uint64_t>> D(m + 1, std::vector<uint64_t>(n + 1, ALN_INF));
    for (int i = 0; i <= m; i++) for (int j = 0; j <= n; j++) {
        if (j - i < lo || j - i > hi) continue;
        if (i == 0 && j == 0) { D[i][j] = 0xFFFFFFFFull; continue; }
        uint64_t v = ALN_INF;
        if (i > 0 && D[i - 1][j] != ALN_INF) v = std::min(v, D[i - 1][j] + ALN_EDIT);
        if (j > 0 && D[i][j - 1] != ALN_INF) v = std::min(v, D[i][j - 1] + ALN_EDIT);
        if (i > 0 && j > 0 && D[i - 1][j - 1] != ALN_INF) v = std::min(v, ((A[i - 1] & 0xDF) == (B[j - 1] & 0xDF)) ? D[i - 1][j - 1] - 1 : D[i - 1][j - 1] + ALN_EDIT);
        D[i][j] = v;
    }
    return D[m][n];
}

int main(int argc, char **argv) {
    const int reps = argc > 1 ? atoi(argv[1]) : 600;
    srand(7);
    const char *alpha = "ACGTacgt";
    long checked = 0;
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
        // make B similar to A sometimes
        if (rand() % 2) {
            for (int x = 0; x < n && x < m; x++) if (rand() % 10) { char c = all[ba + x]; all[strand ? bb + n - 1 - x : bb + x] = strand ? comp(c) : c; }
        }
        int bandmax = rep % 7 == 0 ? 511 : 40;
        uint32_t band = rand() % (bandmax + 1);
        uint32_t nd = align_n_diags(m, n, band);
        if (nd > 1024) continue;
        AlignGeom g = align_geom(m, n, band);
        View va{&all, (uint64_t) ba, (uint64_t) m}, vb{&all, (uint64_t) bb, (uint64_t) n};
        std::string A = all.substr(ba, m), B = all.substr(bb, n);
        if (strand) { std::string R(n, 'A'); for (int x = 0; x < n; x++) R[x] = comp(B[n - 1 - x]); B = R; }
        uint64_t want = brute(A, B, band);
        for (int C : {1, 2, 4, 8}) {
            if (nd > 128u * C) continue;
            uint64_t got = C == 1 ? sim_chain<1>(g, va, vb, strand) : C == 2 ? sim_chain<2>(g, va, vb, strand) : C == 4 ? sim_chain<4>(g, va, vb, strand) : sim_chain<8>(g, va, vb, strand);
            checked++;
            if (got != want) { printf("MISMATCH rep %d C %d m %d n %d band %u strand %u got %llx want %llx\n", rep, C, m, n, band, strand, (unsigned long long) got, (unsigned long long) want); return 1; }
        }
    }
    printf("ok sim_chain_align %ld\n", checked);
    return 0;
}

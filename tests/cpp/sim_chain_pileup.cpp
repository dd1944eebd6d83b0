// sim_chain_pileup -- host only, no device and no libkmu: the functions of kmerutils_amd/csrc/kmu_pile_core.h driven over 64 simulated
// lanes exactly as k_pile_starts and k_pile_vote drive them: the tile starts from the sums of the bases every tile of 64 runs
// consumes, then per tile the scans of the lanes' runs, the votes of every run as a whole from the lane that owns it, and the
// columns 64 at a time, one per lane, through pile_find_run and pile_column.  Checked: every base of A and of B' is stood on by
// exactly one column, every run votes exactly once, every row index lies inside its segment, and the two tables equal a straight
// replay of the runs by the text of include/kmu.h.  pile_call_row is compared with a rule written out the long way.  Random run
// lists on both strands with the run counts at and around the tile size; tests/test_chain_pileup_sim.py builds and runs it; an
// argument sets the number of random cases.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_pile_core.h"
using namespace kmu;

[[noreturn]] static void die(const char *what) {
    printf("FAIL %s\n", what);
    exit(1);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) { // 0 .. n - 1
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) ((rng_state >> 33) % n);
}

typedef std::vector<std::array<uint32_t, PILE_COLS>> Table;

struct Case {
    std::vector<uint32_t> runs;
    uint32_t strand, m, n;
    std::string a, b; // the A segment, and the B segment as it lies on read b (forwards)
};

static uint32_t complement_if(uint32_t strand, uint32_t code) { return strand ? 3u - code : code; }

// the text of include/kmu.h, run by run
static void replay(const Case &c, Table &ta, Table &tb) {
    uint32_t i = 0, j = 0;
    auto pos_b = [&](uint32_t jj) { return c.strand ? c.n - 1u - jj : jj; };
    for (uint32_t run : c.runs) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op == PILE_OP_EQ || op == PILE_OP_X) {
            for (uint32_t k = 0; k < len; k++, i++, j++) {
                ta[i][complement_if(c.strand, pile_code((uint8_t) c.b[pos_b(j)]))]++;
                tb[pos_b(j)][complement_if(c.strand, pile_code((uint8_t) c.a[i]))]++;
            }
        } else if (op == PILE_OP_I) {
            if (c.strand ? j < c.n : j > 0) {
                const uint32_t at = pos_b(c.strand ? j : j - 1u);
                tb[at][PILE_INS]++;
                tb[at][PILE_INS_BASES] += len;
            }
            for (uint32_t k = 0; k < len; k++, i++) ta[i][PILE_DEL]++;
        } else {
            if (i > 0) {
                ta[i - 1][PILE_INS]++;
                ta[i - 1][PILE_INS_BASES] += len;
            }
            for (uint32_t k = 0; k < len; k++, j++) tb[pos_b(j)][PILE_DEL]++;
        }
    }
    if (i != c.m || j != c.n) die("replay does not end at (m, n)");
}

// k_pile_starts and k_pile_vote over 64 lanes; b_start = 0, b_end = n
static void simulate(const Case &c, Table &ta, Table &tb) {
    const uint64_t n_runs = c.runs.size(), n_tiles = pile_n_tiles(n_runs);
    std::vector<std::array<uint32_t, 2>> starts(n_tiles);
    uint64_t si = 0, sj = 0;
    for (uint64_t t = 0; t < n_tiles; t++) { // the starts: the wave's sums, tile by tile
        starts[t] = {(uint32_t) si, (uint32_t) sj};
        for (uint32_t lane = 0; lane < PILE_TILE; lane++) {
            uint32_t da = 0, db = 0;
            if (t * PILE_TILE + lane < n_runs && !pile_run_adv(c.runs[t * PILE_TILE + lane], da, db)) die("a good run is refused");
            si += da;
            sj += db;
        }
        if (si > c.m || sj > c.n) die("the sums pass the segment");
    }
    if (si != c.m || sj != c.n) die("the sums do not end at (m, n)");
    std::vector<uint32_t> seen_a(c.m, 0), seen_b(c.n, 0), seen_run(n_runs, 0);
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t first = t * PILE_TILE;
        const uint32_t nr = n_runs - first < PILE_TILE ? (uint32_t) (n_runs - first) : PILE_TILE;
        uint64_t s_incl[PILE_TILE];
        uint32_t s_run[PILE_TILE], s_i0[PILE_TILE], s_j0[PILE_TILE];
        uint32_t ia = 0, ib = 0, id = 0; // the inclusive scans, lane after lane
        for (uint32_t lane = 0; lane < PILE_TILE; lane++) {
            uint32_t run = 0, da = 0, db = 0;
            if (lane < nr) {
                run = c.runs[first + lane];
                pile_run_adv(run, da, db);
            }
            const uint32_t len = run >> 4;
            ia += da;
            ib += db;
            id += len - da;
            s_incl[lane] = (uint64_t) ia + id;
            s_run[lane] = run;
            s_i0[lane] = starts[t][0] + ia - da;
            s_j0[lane] = starts[t][1] + ib - db;
        }
        for (uint32_t lane = 0; lane < nr; lane++) { // the votes of a run as a whole
            const uint32_t op = s_run[lane] & 15u, len = s_run[lane] >> 4;
            const uint32_t ra = pile_run_row_a(op, s_i0[lane]), rb = pile_run_row_b(op, c.strand, s_j0[lane], c.n);
            seen_run[first + lane]++;
            if (ra != PILE_NONE) {
                if (ra >= c.m) die("a run's row on A is outside the segment");
                ta[ra][PILE_INS]++;
                ta[ra][PILE_INS_BASES] += len;
            }
            if (rb != PILE_NONE) {
                if (rb >= c.n) die("a run's row on B is outside the segment");
                const uint32_t at = pile_b_pos(c.strand, 0, c.n, rb);
                if (at >= c.n) die("a run's position on read b is outside the segment");
                tb[at][PILE_INS]++;
                tb[at][PILE_INS_BASES] += len;
            }
        }
        const uint64_t total = s_incl[PILE_TILE - 1];
        for (uint64_t base = 0; base < total; base += PILE_TILE)
            for (uint32_t lane = 0; lane < PILE_TILE; lane++) {
                const uint64_t col = base + lane;
                if (col >= total) continue;
                const uint32_t r = pile_find_run(s_incl, nr, col);
                if (r >= nr || col >= s_incl[r] || (r && col < s_incl[r - 1])) die("pile_find_run names the wrong run");
                const uint32_t op = s_run[r] & 15u;
                const PileCol pc = pile_column(op, s_i0[r], s_j0[r], (uint32_t) (col - (r ? s_incl[r - 1] : 0)));
                const bool has_a = pc.i != PILE_NONE, has_b = pc.j != PILE_NONE;
                if (!has_a && !has_b) die("a column without a base");
                if (has_a && pc.i >= c.m) die("a column's base of A is outside the segment");
                if (has_b && pc.j >= c.n) die("a column's base of B' is outside the segment");
                const uint32_t at = has_b ? pile_b_pos(c.strand, 0, c.n, pc.j) : 0;
                if (has_b && at >= c.n) die("a column's position on read b is outside the segment");
                if (has_a) {
                    seen_a[pc.i]++;
                    ta[pc.i][has_b ? complement_if(c.strand, pile_code((uint8_t) c.b[at])) : PILE_DEL]++;
                }
                if (has_b) {
                    seen_b[pc.j]++;
                    tb[at][has_a ? complement_if(c.strand, pile_code((uint8_t) c.a[pc.i])) : PILE_DEL]++;
                }
            }
    }
    for (uint32_t v : seen_a)
        if (v != 1) die("a base of A without exactly one column");
    for (uint32_t v : seen_b)
        if (v != 1) die("a base of B' without exactly one column");
    for (uint32_t v : seen_run)
        if (v != 1) die("a run that did not vote exactly once");
}

static Case make_case(uint32_t n_runs, uint32_t max_len, uint32_t strand, int first_op, int last_op) {
    static const uint32_t OPS[4] = {PILE_OP_EQ, PILE_OP_X, PILE_OP_I, PILE_OP_D};
    Case c;
    c.strand = strand;
    c.m = c.n = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        uint32_t op = OPS[rnd(4)];
        if (r == 0 && first_op >= 0) op = OPS[first_op];
        if (r == n_runs - 1 && last_op >= 0) op = OPS[last_op];
        const uint32_t len = rnd(8) == 0 ? 1u + rnd(max_len) : 1u + rnd(9); // adjacent runs may share an op: a cut run
        c.runs.push_back(len << 4 | op);
        uint32_t da, db;
        pile_run_adv(c.runs.back(), da, db);
        c.m += da;
        c.n += db;
    }
    for (uint32_t k = 0; k < c.m; k++) c.a += "ACGTacgt"[rnd(8)];
    for (uint32_t k = 0; k < c.n; k++) c.b += "ACGTacgt"[rnd(8)];
    return c;
}

static uint64_t check_case(const Case &c) {
    Table ta(c.m), tb(c.n), wa(c.m), wb(c.n);
    for (Table *t : {&ta, &tb, &wa, &wb})
        for (auto &row : *t) row.fill(0);
    simulate(c, ta, tb);
    replay(c, wa, wb);
    if (ta != wa) die("the A table differs from the replay");
    if (tb != wb) die("the B table differs from the replay");
    for (const Table *t : {&ta, &tb})
        for (const auto &row : *t)
            if (row[0] + row[1] + row[2] + row[3] + row[PILE_DEL] != 1) die("the depth of a segment row is not 1");
    return c.runs.size();
}

// kmu_pile_call on one row, the long way
static uint32_t call_by_the_text(const uint32_t *row, uint8_t own_byte, uint32_t min_depth) {
    const uint64_t depth = (uint64_t) row[0] + row[1] + row[2] + row[3] + row[4];
    if (depth < min_depth) return 7;
    int own = -1;
    for (int k = 0; k < 4; k++)
        if (own_byte == "ACGT"[k] || own_byte == "acgt"[k]) own = k;
    uint32_t top = 0;
    for (int k = 0; k < 5; k++) top = row[k] > top ? row[k] : top;
    int code = -1;
    if (own >= 0 && row[own] == top) code = own;
    for (int k = 0; k < 5 && code < 0; k++)
        if (row[k] == top) code = k;
    return (uint32_t) code | (2 * (uint64_t) row[5] > depth ? 8u : 0u) | (code != own ? 16u : 0u);
}

int main(int argc, char **argv) {
    const uint32_t n_random = argc > 1 ? (uint32_t) atoi(argv[1]) : 200;
    uint64_t checked = 0;
    const uint32_t counts[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000};
    for (uint32_t n_runs : counts)
        for (uint32_t strand = 0; strand < 2; strand++)
            for (int first = -1; first < 4; first++)
                for (int last = -1; last < 4; last += (first < 0 ? 1 : 4)) checked += check_case(make_case(n_runs, 200, strand, first, last)) + 1;
    for (uint32_t len : {1u, 63u, 64u, 65u, 5000u}) // one run of every op, and an I run then a D run
        for (uint32_t strand = 0; strand < 2; strand++) {
            for (uint32_t op : {PILE_OP_EQ, PILE_OP_X, PILE_OP_I, PILE_OP_D}) {
                Case c = make_case(0, 1, strand, -1, -1);
                c.runs = {len << 4 | op};
                c.m = op == PILE_OP_D ? 0 : len;
                c.n = op == PILE_OP_I ? 0 : len;
                c.a.assign(c.m, 'g');
                c.b.assign(c.n, 'T');
                checked += check_case(c);
            }
            Case c = make_case(0, 1, strand, -1, -1);
            c.runs = {len << 4 | PILE_OP_I, len << 4 | PILE_OP_D};
            c.m = c.n = len;
            c.a.assign(len, 'A');
            c.b.assign(len, 'c');
            checked += check_case(c);
        }
    for (uint32_t rep = 0; rep < n_random; rep++) checked += check_case(make_case(1 + rnd(400), 1 + rnd(300), rep & 1, -1, -1));
    for (uint32_t rep = 0; rep < 20000; rep++) { // the call rule
        uint32_t row[PILE_COLS];
        for (uint32_t &v : row) v = rnd(4) == 0 ? 0xFFFFFFF0u + rnd(16) : rnd(4);
        const uint8_t own = (uint8_t) "ACGTacgtN-"[rnd(10)];
        const uint32_t min_depth = 1 + rnd(6);
        uint64_t depth;
        if (pile_call_row(row, own, min_depth, depth) != call_by_the_text(row, own, min_depth)) die("pile_call_row differs from the text");
        if (depth != (uint64_t) row[0] + row[1] + row[2] + row[3] + row[4]) die("the depth of pile_call_row");
        checked++;
    }
    printf("ok sim_chain_pileup %llu\n", (unsigned long long) checked);
    return 0;
}

// sim_pile_consensus -- host only, no device and no libkmu: the functions of kmerutils_amd/csrc/kmu_cons_core.h driven over 64 simulated
// lanes exactly as k_ins_blocks, k_ins_vote, k_cons_count, k_cons_write and k_cons_offsets drive them.  One chain per case: the A
// segment and the B segment lie in two batches of their own, with other rows before and behind them.  Checked: the block-offset
// lookup equals the full prefix sum on every row; every inserted letter within a row's slots is voted exactly once, into a slot
// inside [S(g), S(g) + ins_len[g]), and the slot tables equal a straight replay of the runs by the text of include/kmu.h; on random
// tables the row lengths of the count pass sum to the total, the bytes of the write pass equal a straight replay, and the read
// offsets equal the replay's.  The slot count is compared with its rule written out the long way.  tests/test_pile_consensus_sim.py
// builds and runs it; an argument sets the number of random cases.  It also runs stand-alone under -fsanitize=address,undefined.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_cons_core.h"
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

typedef std::vector<std::array<uint32_t, CONS_LETTERS>> Slots;

// k_ins_blocks and the scan: block_off[b] = the slots before block b; one more entry: the total
static std::vector<uint64_t> block_offsets(const std::vector<uint8_t> &ins_len) {
    const uint64_t n_blocks = cons_n_blocks(ins_len.size());
    std::vector<uint64_t> off(n_blocks + 1, 0);
    for (uint64_t b = 0; b < n_blocks; b++) {
        uint32_t sum = 0;
        for (uint32_t lane = 0; lane < CONS_BLOCK; lane++) {
            const uint64_t g = b * CONS_BLOCK + lane;
            sum += g < ins_len.size() ? ins_len[g] : 0u;
        }
        off[b + 1] = off[b] + sum;
    }
    return off;
}

static std::vector<uint64_t> prefix(const std::vector<uint8_t> &ins_len) {
    std::vector<uint64_t> s(ins_len.size() + 1, 0);
    for (size_t g = 0; g < ins_len.size(); g++) s[g + 1] = s[g] + ins_len[g];
    return s;
}

static std::vector<uint8_t> random_ins_len(size_t n, uint32_t max_ins) {
    std::vector<uint8_t> v(n, 0);
    for (size_t g = 0; g < n; g++)
        if (rnd(3) == 0) v[g] = (uint8_t) (1u + rnd(max_ins));
    if (n && rnd(2)) v[n - 1] = (uint8_t) max_ins; // slots at the last row of the batch
    if (n && rnd(2)) v[0] = 1;
    return v;
}

static uint64_t n_checked = 0;
static const uint32_t OPS[4] = {PILE_OP_EQ, PILE_OP_X, PILE_OP_I, PILE_OP_D}, CAPS[4] = {1, 2, 16, 255};

// ---- the votes ---------------------------------------------------------------------------------------------------------------------
struct Case {
    std::vector<uint32_t> runs;
    uint32_t strand, m, n;
    std::string a, b;        // the A segment, and the B segment as it lies on read b (forwards)
    uint64_t row_a, row_b;   // the rows of A's base 0 and of the B segment's base 0 in their batches
    std::vector<uint8_t> len_a, len_b;
};

static uint32_t complement_if(uint32_t strand, uint32_t code) { return strand ? 3u - code : code; }

// the text of include/kmu.h, run by run; votes_*: how many letters were voted
static void replay_votes(const Case &c, Slots &sa, Slots &sb, uint64_t &votes_a, uint64_t &votes_b) {
    const std::vector<uint64_t> pa = prefix(c.len_a), pb = prefix(c.len_b);
    uint32_t i = 0, j = 0;
    auto pos_b = [&](uint32_t jj) { return c.strand ? c.n - 1u - jj : jj; };
    for (uint32_t run : c.runs) {
        const uint32_t op = run & 15u, len = run >> 4;
        if (op == PILE_OP_EQ || op == PILE_OP_X) {
            i += len;
            j += len;
        } else if (op == PILE_OP_D) {
            if (i > 0) {
                const uint64_t g = c.row_a + i - 1u;
                for (uint32_t k = 0; k < len && k < c.len_a[g]; k++, votes_a++)
                    sa[pa[g] + k][complement_if(c.strand, pile_code((uint8_t) c.b[pos_b(j + k)]))]++;
            }
            j += len;
        } else {
            if (c.strand ? j < c.n : j > 0) {
                const uint64_t g = c.row_b + pos_b(c.strand ? j : j - 1u);
                for (uint32_t k = 0; k < len && k < c.len_b[g]; k++, votes_b++)
                    sb[pb[g] + k][complement_if(c.strand, pile_code((uint8_t) c.a[c.strand ? i + len - 1u - k : i + k]))]++;
            }
            i += len;
        }
    }
    if (i != c.m || j != c.n) die("replay does not end at (m, n)");
}

// k_ins_vote over 64 lanes; b_start = 0, b_end = n
static void simulate_votes(const Case &c, Slots &sa, Slots &sb, uint64_t &votes_a, uint64_t &votes_b) {
    const std::vector<uint64_t> boff_a = block_offsets(c.len_a), boff_b = block_offsets(c.len_b), pa = prefix(c.len_a), pb = prefix(c.len_b);
    const uint64_t n_runs = c.runs.size(), n_tiles = pile_n_tiles(n_runs);
    uint64_t si = 0, sj = 0;
    for (uint64_t t = 0; t < n_tiles; t++) {
        const uint64_t first = t * PILE_TILE;
        const uint32_t nr = n_runs - first < PILE_TILE ? (uint32_t) (n_runs - first) : PILE_TILE;
        uint32_t ia = 0, ib = 0;
        for (uint32_t lane = 0; lane < nr; lane++) {
            uint32_t da = 0, db = 0;
            const uint32_t run = c.runs[first + lane];
            if (!pile_run_adv(run, da, db)) die("a good run is refused");
            ia += da;
            ib += db;
            const uint32_t op = run & 15u, len = run >> 4, i0 = (uint32_t) si + ia - da, j0 = (uint32_t) sj + ib - db;
            const uint32_t ra = pile_run_row_a(op, i0);
            if (ra != PILE_NONE) {
                if (ra >= c.m || (uint64_t) j0 + len > c.n) die("a D run's row or letters are outside the segments");
                const uint64_t g = c.row_a + ra;
                const uint32_t il = c.len_a[g];
                if (il) {
                    const uint64_t s = cons_slot_base(boff_a.data(), c.len_a.data(), g);
                    if (s != pa[g]) die("the block lookup is not the prefix sum (A)");
                    const uint32_t votes = cons_ins_votes(len, il);
                    if (votes > il || votes > len || s + votes > pa[g + 1]) die("votes beyond the row's slots (A)");
                    for (uint32_t k = 0; k < votes; k++, votes_a++) {
                        const uint32_t src = cons_ins_src_a(j0, k);
                        if (src >= c.n) die("a letter of B' outside the segment");
                        const uint32_t code = cons_ins_code((uint8_t) c.b[pile_b_pos(c.strand, 0, c.n, src)], c.strand);
                        if (code > 3u) die("a letter without a code");
                        sa[s + k][code]++;
                    }
                }
            }
            const uint32_t rb = pile_run_row_b(op, c.strand, j0, c.n);
            if (rb != PILE_NONE) {
                if (rb >= c.n || (uint64_t) i0 + len > c.m) die("an I run's row or letters are outside the segments");
                const uint64_t g = c.row_b + pile_b_pos(c.strand, 0, c.n, rb);
                const uint32_t il = c.len_b[g];
                if (il) {
                    const uint64_t s = cons_slot_base(boff_b.data(), c.len_b.data(), g);
                    if (s != pb[g]) die("the block lookup is not the prefix sum (B)");
                    const uint32_t votes = cons_ins_votes(len, il);
                    if (votes > il || votes > len || s + votes > pb[g + 1]) die("votes beyond the row's slots (B)");
                    for (uint32_t k = 0; k < votes; k++, votes_b++) {
                        const uint32_t src = cons_ins_src_b(c.strand, i0, len, k);
                        if (src < i0 || src >= i0 + len) die("a letter of A outside its run");
                        const uint32_t code = cons_ins_code((uint8_t) c.a[src], c.strand);
                        if (code > 3u) die("a letter without a code");
                        sb[s + k][code]++;
                    }
                }
            }
        }
        si += ia;
        sj += ib;
    }
    if (si != c.m || sj != c.n) die("the sums do not end at (m, n)");
}

static void vote_case(uint32_t n_runs, uint32_t strand, uint32_t max_ins, uint32_t max_len) {
    Case c;
    c.strand = strand;
    c.m = c.n = 0;
    for (uint32_t r = 0; r < n_runs; r++) {
        const uint32_t op = OPS[rnd(4)], len = 1u + rnd(max_len);
        c.runs.push_back(len << 4 | op);
        if (op != PILE_OP_D) c.m += len;
        if (op != PILE_OP_I) c.n += len;
    }
    const char *letters = rnd(2) ? "ACGT" : "acgt";
    for (uint32_t k = 0; k < c.m; k++) c.a += letters[rnd(4)];
    for (uint32_t k = 0; k < c.n; k++) c.b += letters[rnd(4)];
    c.row_a = rnd(130);
    c.row_b = rnd(130);
    c.len_a = random_ins_len(c.row_a + c.m + rnd(70), max_ins);
    c.len_b = random_ins_len(c.row_b + c.n + rnd(70), max_ins);
    const std::vector<uint64_t> pa = prefix(c.len_a), pb = prefix(c.len_b);
    Slots sa(pa.back()), sb(pb.back()), ra(pa.back()), rb(pb.back());
    for (Slots *s : {&sa, &sb, &ra, &rb})
        for (auto &x : *s) x.fill(0);
    uint64_t va = 0, vb = 0, wa = 0, wb = 0;
    simulate_votes(c, sa, sb, va, vb);
    replay_votes(c, ra, rb, wa, wb);
    if (va != wa || vb != wb) die("the number of voted letters differs from the replay's");
    if (sa != ra || sb != rb) die("the slot tables differ from the replay's");
    n_checked += n_runs + va + vb;
}

// ---- the block lookup on every row ----------------------------------------------------------------------------------------------
static void lookup_case(size_t n_rows, uint32_t max_ins) {
    const std::vector<uint8_t> len = random_ins_len(n_rows, max_ins);
    const std::vector<uint64_t> boff = block_offsets(len), p = prefix(len);
    if (boff.back() != p.back()) die("the block offsets do not end at the total");
    for (size_t g = 0; g < n_rows; g++)
        if (cons_slot_base(boff.data(), len.data(), g) != p[g]) die("the block lookup is not the prefix sum");
    n_checked += n_rows;
}

// ---- the slot count ----------------------------------------------------------------------------------------------------------------
static void slot_count_cases() {
    for (uint32_t rep = 0; rep < 20000; rep++) {
        uint32_t row[PILE_COLS];
        const bool big = rnd(50) == 0;
        for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = big && rnd(2) ? 0xFFFFFFFFu - rnd(3) : rnd(rnd(2) ? 4 : 40);
        const uint32_t max_ins = CAPS[rnd(4)], call = rnd(32);
        uint64_t depth = 0;
        for (uint32_t k = 0; k < 5; k++) depth += row[k];
        uint64_t want = 0; // the largest k <= max_ins with k * depth < 2 * INS_BASES
        if ((call & PILE_CALL_INS) && depth)
            while (want < max_ins && (want + 1u) * depth < 2ull * row[PILE_INS_BASES]) want++;
        if (cons_slot_count(row, call, max_ins) != want) die("cons_slot_count differs from its rule");
        if (cons_depth(row) != depth) die("cons_depth");
    }
    n_checked += 20000;
}

// ---- the consensus -------------------------------------------------------------------------------------------------------------------
static void consensus_case(const std::vector<uint32_t> &read_len, uint32_t max_ins) {
    std::vector<uint64_t> off(1, 0);
    for (uint32_t l : read_len) off.push_back(off.back() + l);
    const uint64_t n_rows = off.back(), n_tiles = cons_n_blocks(n_rows);
    const std::vector<uint8_t> len = random_ins_len(n_rows, max_ins);
    const std::vector<uint64_t> slot_off = block_offsets(len), p = prefix(len);
    std::vector<std::array<uint32_t, PILE_COLS>> pile(n_rows);
    std::vector<uint8_t> call(n_rows), bases(n_rows);
    Slots ins(p.back());
    for (uint64_t g = 0; g < n_rows; g++) {
        for (uint32_t k = 0; k < PILE_COLS; k++) pile[g][k] = rnd(4);
        call[g] = (uint8_t) (rnd(4) == 0 ? rnd(32) : rnd(2) ? PILE_CALL_NONE : rnd(5) | (rnd(2) ? PILE_CALL_INS : 0u));
        bases[g] = (uint8_t) "ACGTacgtNn-"[rnd(11)];
    }
    for (auto &s : ins)
        for (uint32_t x = 0; x < CONS_LETTERS; x++) s[x] = rnd(5) == 0 ? 0u : rnd(6); // not monotone along a row's slots
    const uint32_t *ins_words = ins.empty() ? nullptr : ins[0].data();

    // the straight replay, by the text of include/kmu.h
    std::vector<uint8_t> want;
    std::vector<uint64_t> row_end(n_rows + 1, 0);
    for (uint64_t g = 0; g < n_rows; g++) {
        const uint32_t code = call[g] & 7u;
        if (code < 4u) want.push_back((uint8_t) "ACGT"[code]);
        else if (code != PILE_DEL) want.push_back(bases[g]);
        uint64_t depth = 0;
        for (uint32_t k = 0; k < 5; k++) depth += pile[g][k];
        for (uint32_t k = 0; k < len[g]; k++) {
            const auto &s = ins[p[g] + k];
            if (2ull * ((uint64_t) s[0] + s[1] + s[2] + s[3]) <= depth) break;
            uint32_t best = 0;
            for (uint32_t x = 1; x < 4; x++)
                if (s[x] > s[best]) best = x;
            want.push_back((uint8_t) "ACGT"[best]);
        }
        row_end[g + 1] = want.size();
    }

    // k_cons_count: one row per lane, the tile sums; the scan
    auto row_at = [&](uint64_t g, uint64_t slot, uint8_t *out) {
        if (slot != p[g]) die("a row's first slot is not the prefix sum");
        return cons_row(call[g], out ? bases[g] : 0u, len[g], pile[g].data(), ins_words ? ins_words + slot * CONS_LETTERS : nullptr, out);
    };
    std::vector<uint64_t> tile_off(n_tiles + 1, 0);
    uint64_t sum_rows = 0;
    for (uint64_t t = 0; t < n_tiles; t++) {
        uint32_t sum = 0, scan = 0;
        for (uint32_t lane = 0; lane < CONS_BLOCK; lane++) {
            const uint64_t g = t * CONS_BLOCK + lane;
            if (g >= n_rows) continue;
            const uint32_t n = row_at(g, slot_off[t] + scan, nullptr);
            if (n > 1u + len[g]) die("a row longer than its position and its slots");
            scan += len[g];
            sum += n;
            sum_rows += n;
        }
        tile_off[t + 1] = tile_off[t] + sum;
    }
    if (sum_rows != want.size() || tile_off[n_tiles] != want.size()) die("the row lengths do not sum to the total");

    // k_cons_write: the wave's prefix sum, every lane stores its row; canaries on both sides
    std::vector<uint8_t> got(want.size() + 2, 0xEE);
    for (uint64_t t = 0; t < n_tiles; t++) {
        uint32_t scan = 0, at = 0;
        for (uint32_t lane = 0; lane < CONS_BLOCK; lane++) {
            const uint64_t g = t * CONS_BLOCK + lane;
            if (g >= n_rows) continue;
            const uint32_t n = row_at(g, slot_off[t] + scan, nullptr);
            if (tile_off[t] + at + n > want.size()) die("a row's bytes end beyond the total");
            if (n && row_at(g, slot_off[t] + scan, got.data() + 1 + tile_off[t] + at) != n) die("the write pass counts differently");
            scan += len[g];
            at += n;
        }
    }
    if (got.front() != 0xEE || got.back() != 0xEE) die("a byte outside the output");
    if (!std::equal(want.begin(), want.end(), got.begin() + 1)) die("the written bytes differ from the replay's");

    // k_cons_offsets: one lane per read, and one for the end
    for (size_t r = 0; r < off.size(); r++) {
        const uint64_t g0 = off[r], t = g0 / CONS_BLOCK;
        uint64_t at = tile_off[t], slot = slot_off[t];
        for (uint64_t g = t * CONS_BLOCK; g < g0; g++) {
            at += row_at(g, slot, nullptr);
            slot += len[g];
        }
        if (at != row_end[g0]) die("a read's offset differs from the replay's");
    }
    n_checked += n_rows + want.size();
}

int main(int argc, char **argv) {
    const uint32_t reps = argc > 1 ? (uint32_t) atoi(argv[1]) : 100;
    slot_count_cases();
    const uint32_t sizes[] = {0, 1, 2, 63, 64, 65, 127, 128, 129, 1000};
    const uint32_t caps[] = {1, 16, 255};
    for (uint32_t n : sizes)
        for (uint32_t cap : caps) {
            lookup_case(n, cap);
            for (uint32_t strand = 0; strand < 2; strand++) {
                vote_case(n, strand, cap, 12);
                vote_case(n / 8 + 1, strand, cap, 300); // runs longer than any slot count
            }
            consensus_case({n}, cap);
            consensus_case({0, n / 2, 0, 0, n - n / 2, 0}, cap);
            consensus_case({3, n, 61, 64, 1, n}, cap);
        }
    for (uint32_t rep = 0; rep < reps; rep++) {
        const uint32_t cap = caps[rnd(3)];
        vote_case(rnd(200), rnd(2), cap, 1u + rnd(40));
        lookup_case(rnd(700), cap);
        std::vector<uint32_t> lens;
        for (uint32_t r = rnd(8); r > 0; r--) lens.push_back(rnd(3) ? rnd(200) : 0);
        consensus_case(lens, cap);
    }
    printf("ok sim_pile_consensus %llu\n", (unsigned long long) n_checked);
    return 0;
}

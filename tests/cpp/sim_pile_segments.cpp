// sim_pile_segments -- host only, no device and no libkmu: the functions of kmerutils_amd/csrc/kmu_seg_core.h and kmu_gather_core.h
// (the copy: sim_gather.h) driven over 64 simulated lanes exactly as k_seg_marks, k_seg_count, k_seg_write, k_seg_keep, k_seg_reads and k_ext_copy drive them.  Random tables over
// random read lengths (empty reads, reads of many tiles, depths around min_depth, ENDS around the depth).  Checked: every tile counts
// in the write pass what it counted in the count pass; starts and ends pair up (as many, the k-th start below the k-th end, the k-th
// end at or below the start after it); the runs equal a straight per-read replay of the text of include/kmu.h; every row is in at most
// one run, and every good row in exactly one; no run crosses a read boundary; the summaries equal the replay's.  For the copy: every
// output byte is written exactly once, from the byte the offsets name.  tests/test_pile_segments_sim.py builds and runs it; an
// argument sets the number of random cases.  It also runs stand-alone under -fsanitize=address,undefined.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../kmerutils_amd/csrc/kmu_seg_core.h"
#include "sim_gather.h"
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

static uint64_t n_checked = 0;
typedef std::vector<std::array<uint32_t, PILE_COLS>> Table;
struct Rule {
    uint32_t min_depth, min_span, min_len;
};
struct ReadSum {
    uint32_t n_bases, n_good, n_segs, kept, best_start, best_end, inner_bad, cls;
    bool operator==(const ReadSum &o) const {
        return n_bases == o.n_bases && n_good == o.n_good && n_segs == o.n_segs && kept == o.kept && best_start == o.best_start && best_end == o.best_end &&
               inner_bad == o.inner_bad && cls == o.cls;
    }
};

// the text of include/kmu.h, read by read
static void replay(const Table &pile, const std::vector<uint64_t> &off, const Rule &rule, std::vector<std::pair<uint64_t, uint64_t>> &runs,
                   std::vector<ReadSum> &sums) {
    auto depth = [&](uint64_t g) { return (uint64_t) pile[g][0] + pile[g][1] + pile[g][2] + pile[g][3] + pile[g][4]; };
    auto span = [&](uint64_t g) { return depth(g) > pile[g][PILE_ENDS] ? depth(g) - pile[g][PILE_ENDS] : 0ull; };
    for (size_t r = 0; r + 1 < off.size(); r++) {
        ReadSum s{(uint32_t) (off[r + 1] - off[r]), 0, 0, 0, 0, 0, 0, SEG_NONE};
        uint32_t first = 0, last = 0;
        for (uint64_t g = off[r]; g < off[r + 1];) {
            if (depth(g) < rule.min_depth) {
                g++;
                continue;
            }
            const uint64_t b = g++;
            while (g < off[r + 1] && depth(g) >= rule.min_depth && std::max(span(g), span(g - 1)) >= rule.min_span) g++;
            runs.push_back({b, g});
            s.n_good += (uint32_t) (g - b);
            if (g - b < rule.min_len) continue;
            const uint32_t st = (uint32_t) (b - off[r]), en = (uint32_t) (g - off[r]);
            if (s.n_segs == 0) first = st;
            last = en;
            if (en - st > s.best_end - s.best_start) s.best_start = st, s.best_end = en;
            s.n_segs++;
            s.kept += en - st;
        }
        s.inner_bad = s.n_segs ? last - first - s.kept : 0;
        s.cls = s.n_segs == 0 ? SEG_NONE : s.n_segs > 1 ? SEG_SPLIT : s.kept == s.n_bases ? SEG_WHOLE : SEG_ENDS;
        sums.push_back(s);
    }
}

// k_seg_tiles over 64 lanes: counts only, or the compacted starts and ends at the tile's offsets
static void tile_pass(const Table &pile, uint64_t n_rows, const std::vector<uint64_t> &marks, const Rule &rule, uint64_t t, uint32_t &ns_out, uint32_t &ne_out,
                      const std::vector<uint64_t> *soff, const std::vector<uint64_t> *eoff, std::vector<uint64_t> *starts, std::vector<uint64_t> *ends) {
    const uint64_t base = t * SEG_TILE;
    SegRow carry = base > 0 && base - 1 < n_rows ? seg_row(pile[base - 1].data(), rule.min_depth) : seg_no_row();
    uint32_t ns = 0, ne = 0;
    for (uint32_t trip = 0; trip < SEG_TRIPS; trip++) {
        const uint64_t g0 = base + (uint64_t) trip * 64u;
        if (g0 > n_rows) break;
        SegRow cur[64];
        for (uint32_t lane = 0; lane < 64; lane++) cur[lane] = g0 + lane < n_rows ? seg_row(pile[g0 + lane].data(), rule.min_depth) : seg_no_row();
        if ((g0 >> 6) >= marks.size()) die("a mark word outside the bitmap");
        for (uint32_t lane = 0; lane < 64; lane++) {
            const uint64_t g = g0 + lane;
            const SegRow prev = lane ? cur[lane - 1] : carry;
            const bool marked = (marks[g0 >> 6] >> lane) & 1ull;
            if (g <= n_rows && marked != seg_marked(marks.data(), g)) die("seg_marked differs from the word's bit");
            const bool st = seg_is_start(prev, cur[lane], marked, rule.min_span), en = seg_is_end(prev, cur[lane], st);
            if ((st || en) && g > n_rows) die("a start or an end beyond position n_rows");
            if (st && starts) {
                if ((*soff)[t] + ns >= starts->size()) die("a start beyond the number of runs");
                (*starts)[(*soff)[t] + ns] = g;
            }
            if (en && ends) {
                if ((*eoff)[t] + ne >= ends->size()) die("an end beyond the number of runs");
                (*ends)[(*eoff)[t] + ne] = g;
            }
            ns += st;
            ne += en;
        }
        carry = cur[63];
    }
    ns_out = ns;
    ne_out = ne;
}

static void segment_case(const std::vector<uint32_t> &read_len, const Rule &rule, uint32_t max_count) {
    std::vector<uint64_t> off(1, 0);
    for (uint32_t l : read_len) off.push_back(off.back() + l);
    const uint64_t n_rows = off.back(), n_tiles = seg_n_tiles(n_rows);
    const uint32_t n_reads = (uint32_t) read_len.size();
    Table pile(n_rows);
    const bool big = rnd(8) == 0;
    for (auto &row : pile) {
        for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = rnd(max_count);
        if (rnd(3) == 0) row[PILE_ENDS] = 0;
        if (big && rnd(4) == 0) row[0] = 0xFFFFFFFFu - rnd(2), row[1] = rnd(3); // depths around 2^32
        if (rnd(40) == 0)
            for (uint32_t k = 0; k < 5; k++) row[k] = 0;
    }
    // k_seg_marks
    std::vector<uint64_t> marks(n_rows / 64 + 1, 0);
    for (uint32_t r = 0; r < n_reads; r++)
        if (off[r] <= n_rows) marks[off[r] >> 6] |= 1ull << (off[r] & 63);
    // k_seg_count, the scans, k_seg_write
    std::vector<uint64_t> soff(n_tiles + 1, 0), eoff(n_tiles + 1, 0);
    for (uint64_t t = 0; t < n_tiles; t++) {
        uint32_t ns, ne;
        tile_pass(pile, n_rows, marks, rule, t, ns, ne, nullptr, nullptr, nullptr, nullptr);
        soff[t + 1] = soff[t] + ns;
        eoff[t + 1] = eoff[t] + ne;
    }
    if (soff[n_tiles] != eoff[n_tiles]) die("starts and ends differ in number");
    const uint64_t n_runs = soff[n_tiles];
    std::vector<uint64_t> starts(n_runs, ~0ull), ends(n_runs, ~0ull);
    for (uint64_t t = 0; t < n_tiles; t++) {
        uint32_t ns, ne;
        tile_pass(pile, n_rows, marks, rule, t, ns, ne, &soff, &eoff, &starts, &ends);
        if (ns != soff[t + 1] - soff[t] || ne != eoff[t + 1] - eoff[t]) die("the write pass counts differently");
    }
    // the pairing, the replay
    std::vector<std::pair<uint64_t, uint64_t>> want;
    std::vector<ReadSum> want_sums;
    replay(pile, off, rule, want, want_sums);
    if (want.size() != n_runs) die("the number of runs differs from the replay's");
    std::vector<uint8_t> covered(n_rows, 0);
    for (uint64_t k = 0; k < n_runs; k++) {
        if (!(starts[k] < ends[k] && ends[k] <= n_rows)) die("a start that is not below its end");
        if (k + 1 < n_runs && ends[k] > starts[k + 1]) die("a run that overlaps the next");
        if (starts[k] != want[k].first || ends[k] != want[k].second) die("a run differs from the replay's");
        for (uint64_t g = starts[k]; g < ends[k]; g++)
            if (covered[g]++) die("a row in two runs");
    }
    for (uint64_t g = 0; g < n_rows; g++)
        if ((seg_row(pile[g].data(), rule.min_depth).good != 0) != (covered[g] != 0)) die("a good row outside every run, or a bad row inside one");
    // k_seg_keep, the scan of the reads' counts, k_seg_place, k_seg_reads
    std::vector<uint32_t> n_good(n_reads, 0), n_kept(n_reads, 0);
    std::vector<std::array<uint32_t, 3>> kept; // read, start, end
    for (uint64_t k = 0; k < n_runs; k++) {
        const uint32_t r = (uint32_t) gather_upper_index(off.data(), n_reads, starts[k]);
        if (r >= n_reads || off[r] > starts[k] || off[r + 1] <= starts[k]) die("gather_upper_index names a read that does not hold the row");
        if (ends[k] > off[r + 1]) die("a run crosses a read boundary");
        const uint32_t len = (uint32_t) (ends[k] - starts[k]);
        n_good[r] += len;
        if (len >= rule.min_len) {
            n_kept[r]++;
            kept.push_back({r, (uint32_t) (starts[k] - off[r]), (uint32_t) (ends[k] - off[r])});
        }
    }
    uint64_t at = 0;
    for (uint32_t r = 0; r < n_reads; r++) {
        SegSummary s = seg_summary_begin();
        for (uint32_t i = 0; i < n_kept[r]; i++, at++) {
            if (kept[at][0] != r) die("a read's kept segments are not where the scan of its count says");
            seg_summary_add(s, kept[at][1], kept[at][2]);
        }
        const ReadSum got{(uint32_t) (off[r + 1] - off[r]), n_good[r], s.n_segs, s.kept, s.best_start, s.best_end, seg_inner_bad(s), seg_class(s, (uint32_t) (off[r + 1] - off[r]))};
        if (!(got == want_sums[r])) die("a read's summary differs from the replay's");
        if (s.n_segs && !(kept[at - s.n_segs + s.best_rank][1] == s.best_start && kept[at - s.n_segs + s.best_rank][2] == s.best_end)) die("best_rank does not name the best");
    }
    if (at != kept.size()) die("kept segments left over");
    n_checked += n_rows + n_runs;
}

// k_ext_copy over 64 lanes: the walk of sim_gather.h over the ranges' offsets
static void copy_case(const std::vector<uint32_t> &len) {
    std::vector<uint64_t> off(1, 0);
    for (uint32_t l : len) off.push_back(off.back() + l);
    uint64_t n_bytes = 0;
    gather_replay(off, die, [&](uint64_t, uint64_t) { n_bytes++; });
    if (n_bytes != off.back()) die("the copy delivers another number of bytes than the offsets name");
    n_checked += off.back() + len.size();
}

int main(int argc, char **argv) {
    const uint32_t reps = argc > 1 ? (uint32_t) atoi(argv[1]) : 100;
    const uint32_t T = SEG_TILE;
    const uint32_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 5 * T + 3};
    const Rule rules[] = {{1, 0, 1}, {3, 0, 1}, {3, 3, 1}, {3, 2, 5}, {2, 7, 64}, {0xFFFFFFFFu, 1, 1}};
    for (uint32_t n : sizes)
        for (const Rule &rule : rules) {
            segment_case({n}, rule, 3);
            segment_case({0, n / 2, 0, 0, n - n / 2, 0}, rule, 4);
            segment_case({T - n % T, n, 61, 64, 1, n}, rule, 6);
        }
    // ends that are never hit, and find_read on reads of 0 to 3 rows
    std::vector<uint32_t> tiny;
    for (uint32_t r = 0; r < 2000; r++) tiny.push_back(rnd(4));
    segment_case(tiny, {1, 0, 1}, 3);
    segment_case(tiny, {2, 1, 2}, 3);
    for (uint32_t rep = 0; rep < reps; rep++) {
        std::vector<uint32_t> lens;
        for (uint32_t r = rnd(9); r > 0; r--) lens.push_back(rnd(3) ? rnd(rnd(4) ? 200 : 3000) : 0);
        segment_case(lens, {1 + rnd(4), rnd(5), 1 + rnd(rnd(2) ? 3 : 80)}, 2 + rnd(4));
    }
    copy_case({});
    copy_case({0, 0, 0});
    copy_case({GATHER_TILE * 3 + 5});
    copy_case(std::vector<uint32_t>(5000, 1));
    {
        std::vector<uint32_t> l(300, 0); // more than 64 empty ranges in a row, in front, inside and behind
        l[100] = 7;
        l[250] = GATHER_TILE;
        copy_case(l);
    }
    for (uint32_t rep = 0; rep < reps; rep++) {
        std::vector<uint32_t> l;
        for (uint32_t r = rnd(400); r > 0; r--) l.push_back(rnd(3) == 0 ? 0 : rnd(5) == 0 ? rnd(9000) : rnd(40));
        copy_case(l);
    }
    printf("ok sim_pile_segments %llu\n", (unsigned long long) n_checked);
    return 0;
}

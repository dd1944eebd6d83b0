// kmu_count_part.hip -- the host side of the radix-partitioned build of the count table (the throughput path of
// kmu_count_add_reads / kmu_sketch_count): big batches never touch the table with atomics, HBM sees only streams.  The kernels
// are in kmu_count_part_{level1,array,build}.hip (declared in kmu_count_part_kernels.h), the arithmetic of the plans in kmu_count_plan.hpp.
// Every stage has ONE host function here and the routes are made of them: the SINGLE-PASS partition (default for big batches:
// no histogram passes; seg_buffers, a level 1, seg_tails, seg_level2_build) and, where its spill list fills up, the EXACT levels
// (reads_census, reads_scatter_exact, arr_level_exact; also one-level tables, the owner grouping of a distributed add with
// hash owners, the generic array partition of the sketch path); both end in launch_build.
#include <algorithm>
#include <vector>

#include "kmu_count_part_kernels.h"
#include "kmu_count_plan.hpp"
#include "kmu_flat.h"

namespace kmu {

// ---- what every route ends in, or needs ----------------------------------------------------------------------------------
static size_t build_lds(const kmu_counter *c) { return c->qw ? (size_t) 8 << c->rbits : (size_t) 12 << c->rbits; }
static size_t build_pool_lds(const kmu_counter *c) { return c->qw ? (size_t) (BUILD_THREADS / 64) * BUILD_POOL * 8 : 0; } // (k_part_build_q's pools)
// the items of every region (leaves: the regions' bounds; or leaf_stride / leafcnt: fixed-size leaves with their fills) into the table
template <int IT>
static int launch_build(kmu_counter *c, const uint64_t *items, const uint64_t *leaves, uint32_t *d_err,
                        uint64_t leaf_stride = 0, const uint32_t *leafcnt = nullptr, bool leaf6 = false) {
    kmu_ctx *ctx = c->ctx;
    const uint64_t n_regions = table_regions(c);
    const int in_mode = c->empty ? 0 : 1;
    const size_t lds = build_lds(c) + build_pool_lds(c);
    const int per_cu = c->qw ? std::min(32 / (BUILD_THREADS / 64), (int) ((160 * 1024) / lds)) : 3;
    const int grid = grid_for(ctx, n_regions, 1, per_cu * 8);
    {
        const auto kern = !c->qw ? k_part_build<IT> : leaf6 ? k_part_build_q<IT_HASH, true> : k_part_build_q<IT, false>;
        KMU_TRY(launch(ctx, c->qw ? "k_part_build_q" : "k_part_build", kern, dim3(grid), dim3(BUILD_THREADS), lds, items, leaves,
                       (uint32_t) n_regions, table_of(c), in_mode, d_err, leaf_stride, leafcnt));
    }
    c->empty = false;
    return KMU_OK;
}
// the LDS-staged scatter kernels ask for more than 64 KiB of dynamic LDS: one attribute call per instantiation and device
// (function attributes are per device: remembered per context, not per process)
static int scatter_attrs(kmu_ctx *ctx) {
    if (ctx->lds_attr_set & 1u) return KMU_OK;
    const void *fns[] = {(const void *) k_part_scatter1_exact, (const void *) k_part_scatter1,
                         (const void *) k_arr_scatter_exact<IT_HASH>, (const void *) k_arr_scatter_exact<IT_KEY>, (const void *) k_arr_scatter_exact<IT_KEY_TO_HASH>,
                         (const void *) k_arr_scatter_seg<IT_HASH, false>, (const void *) k_arr_scatter_seg<IT_HASH, true>,
                         (const void *) k_arr_scatter_seg<IT_KEY_TO_HASH, false>, (const void *) k_smer_scatter1};
    for (const void *f : fns) KMU_HIP(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ctx->lds_attr_set |= 1u;
    return KMU_OK;
}
// the partition plan of a table: its own region map
bool part_plan_for(const kmu_counter *c, PartPlan *pl) {
    memset(pl, 0, sizeof *pl);
    pl->b1 = c->b1;
    pl->n2 = c->n2;
    return c->b1 <= 11 && c->n2 <= GROUP_REGIONS_MAX;
}

// ---- the single-pass partition -------------------------------------------------------------------------------------------
// The k-mers travel as khash(k-mer), so the digits are uniform: a stream's share of the items is items / bins with a standard
// deviation of sqrt(that).  Every stream gets a FIXED capacity of mean + 5 sigma + 32 items (1.4 % over the mean at level 1 of
// the bench size, 13 % per region leaf), the scatters run without their histogram passes (-7.6 and -6.0 ms), the unused tail of
// every level-1 stream is filled with "no k-mer" marks that level 2 skips, the leaves carry their fill in a count of their own.
// An item that finds its stream full goes to a spill list that is inserted into the finished table (seg_spill,
// k_count_add_spill); only a full spill list (k-mers that the hash cannot spread: a genome of one repeated k-mer) raises a flag
// that is read before the build touches the table: the call then takes the exact route from scratch.  Level 1 without a global
// histogram is also what lets kmu_sketch_count partition a chunk while the next one is uploaded.
bool seg_partition_wanted(uint64_t n_items) {
    const char *e = getenv("KMU_COUNT_SEG"); // 0: always the exact two-pass levels; 2: also for small batches (tests)
    if (e && atoi(e) == 0) return false;
    if (e && atoi(e) == 2) return true;
    if (n_items >> 35) return false; // (positions inside a level-1 bin and the cursors of the shared streams are 32-bit numbers:
                                     //  a set of streams sees at most n / sets items, whatever their bins)
    // (with streams shared by a set's units the route wins wherever a table has two levels: 5.9 / 8.8 / 17.6 / 35 / 70 Mbases:
    //  0.22 / 0.27 / 0.40 / 0.66 / 1.14 ms against 0.65 / 0.70 / 0.83 / 1.14 / 1.68 for the exact levels, scripts/r03_segthr.sh)
    return n_items >= (1ull << 22);
}
// the share of mean + 5 sigma a stream gets (seg_cap_for); KMU_COUNT_SEG_PCT: tests, force overflows
static double seg_cap_share() {
    const char *e = getenv("KMU_COUNT_SEG_PCT");
    return e ? std::max(0.01, atof(e) / 100.0) : 1.0;
}
// 6-byte leaf items instead of 8: a table whose slots keep <= 48 bits of an item (w >= 16); KMU_COUNT_LEAF6=0: tests
static bool leaf6_wanted(const kmu_counter *c) {
    bool on = true;
    if (const char *e = getenv("KMU_COUNT_LEAF6")) on = atoi(e) != 0;
    return on && c->qw >= 16 && c->n2 <= LEAF6_MAX_BINS;
}

// The buffers of a single-pass partition of n_items items: level 1's streams A, the leaves B with their fills, the overflow word
// block (see seg_spill) with its spill list (room for 1/32 of the items), the cursors of the streams (zero).  own_buffer: A must
// survive other users of the shared scratch "cnt.partA" (kmu_sketch_count's chunked form: the sketch of the next chunk writes
// its (key, weight) lists there while this partition is still being filled)
struct SegBufs { void *A = nullptr, *B = nullptr, *leafcnt = nullptr, *ovf = nullptr, *spill = nullptr, *state = nullptr; };
static int seg_buffers(kmu_ctx *ctx, const PartPlan &pl, const SegPlan &sp, uint64_t n_items, bool own_buffer, SegBufs *b) {
    const uint32_t bins1 = plan_bins1(pl);
    const uint64_t n_regions = plan_regions(pl);
    // (+ two tiles: level 2 requests whole tiles a tile ahead: its last request of the last bin ends less than two tiles behind the bin)
    KMU_TRY(dev_buf(ctx, own_buffer ? "cnt.segA" : "cnt.partA", (size_t) bins1 * sp.sets * sp.cap1 * 8 + (size_t) 2 * TILE_ITEMS * 8 + 64, &b->A));
    KMU_TRY(dev_buf(ctx, "cnt.partB", (size_t) n_regions * sp.cap2 * 8 + 64, &b->B));
    KMU_TRY(dev_buf(ctx, "cnt.leafcnt", (size_t) n_regions * 4 + 64, &b->leafcnt));
    const uint64_t spill_cap = std::min<uint64_t>(n_items / 32 + 4096, 0x7FFFFFFFull);
    KMU_TRY(dev_buf(ctx, "cnt.seg_ovf", 64, &b->ovf));
    KMU_TRY(dev_buf(ctx, "cnt.spill", (size_t) spill_cap * 8 + 64, &b->spill));
    KMU_TRY(launch(ctx, nullptr, k_spill_header, dim3(1), dim3(64), 0, (uint32_t *) b->ovf, (uint32_t) spill_cap, (uint64_t *) b->spill));
    KMU_TRY(dev_buf(ctx, "cnt.seg_state", (size_t) sp.sets * bins1 * 4 + 64, &b->state));
    KMU_HIP(ctx, hipMemsetAsync(b->state, 0, (size_t) sp.sets * bins1 * 4, ctx->stream));
    return scatter_attrs(ctx);
}
// behind the last launch of a level 1: "no k-mer" marks from the fill of every (set, bin) stream to its capacity
static int seg_tails(kmu_ctx *ctx, const PartPlan &pl, const SegPlan &sp, const SegBufs &b) {
    const uint32_t n_streams = sp.sets * plan_bins1(pl);
    KMU_TRY(launch(ctx, nullptr, k_seg_tails, dim3(grid_for(ctx, n_streams, 1)), dim3(256), 0,
                   (const uint32_t *) b.state, n_streams, (uint32_t) sp.cap1, (uint64_t *) b.A));
    return KMU_OK;
}
// The tail of a single-pass partition: level 2 (A, level 1's streams -> the leaves in B, SEG_L2_UNITS units per bin sharing its
// leaves), the overflow words, the build, the spilled items.  *taken = 0: the spill list overflowed and the table is untouched
// (the words are read BEFORE the build): the caller takes the exact route from scratch.
static int seg_level2_build(kmu_counter *c, const PartPlan &pl, const SegPlan &sp, const SegBufs &b, uint32_t *d_err, int *taken) {
    kmu_ctx *ctx = c->ctx;
    *taken = 0;
    const uint32_t bins1 = plan_bins1(pl);
    const bool leaf6 = leaf6_wanted(c);
    const ArrPlan ap{plan_digit2(pl), pl.n2, bins1, SEG_L2_UNITS, sp.sets, (uint32_t) sp.cap1, bins1, 0u};
    KMU_HIP(ctx, hipMemsetAsync(b.leafcnt, 0, (size_t) ap.nparts * ap.bins * 4, ctx->stream));
    {
        const auto k2 = leaf6 ? k_arr_scatter_seg<IT_HASH, true> : k_arr_scatter_seg<IT_HASH, false>;
        KMU_TRY(launch(ctx, "k_arr_scatter", k2, dim3(ap.nparts * ap.chunks), dim3(SCATTER_THREADS), seg_lds_bytes(ap.bins, leaf6),
                       (const uint64_t *) b.A, (const uint64_t *) nullptr, ap, (uint64_t *) b.B, sp.cap2, (uint32_t *) b.ovf, (uint32_t *) b.leafcnt,
                       (const uint32_t *) c->lox));
    }
    uint32_t h_ovf[2] = {0, 0}; // [0] the list is full, [1] items spilled
    KMU_HIP(ctx, hipMemcpyAsync(h_ovf, b.ovf, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_ovf[0]) return KMU_OK;
    KMU_TRY(launch_build<IT_HASH>(c, (const uint64_t *) b.B, nullptr, d_err, sp.cap2, (const uint32_t *) b.leafcnt, leaf6));
    if (h_ovf[1]) {
        KMU_TRY(launch(ctx, "k_count_add_spill", k_count_add_spill, dim3(grid_for(ctx, h_ovf[1], 256)), dim3(256), 0, (const uint64_t *) b.spill,
                       (const uint32_t *) b.ovf, table_of(c), d_err));
    }
    *taken = 1;
    return KMU_OK;
}

// state of a single-pass partition of reads between its level-1 launches (kmu_sketch_count runs them chunk by chunk under the upload)
struct SegRun {
    PartPlan pl;
    SegPlan sp;
    DevSeqs ds;
    uint64_t total_bases = 0;
    uint64_t steps_done = 0; // wave steps of the stream that have been through level 1
    bool l1_done = false;
    SegBufs b;
    void *novalid = nullptr;
    uint32_t *d_err = nullptr;
};
static int seg_begin(kmu_counter *c, const DevSeqs &ds, uint64_t total_bases, const PartPlan &pl_in, uint32_t *d_err, SegRun *run,
                     bool own_buffer = false) {
    kmu_ctx *ctx = c->ctx;
    const SegPlan sp = seg_plan((uint32_t) ctx->num_cus, total_bases, plan_bins1(pl_in), pl_in.n2, seg_cap_share());
    *run = SegRun{pl_in, sp, ds, total_bases, 0, false, SegBufs{}, nullptr, d_err};
    run->pl.units1 = run->sp.units1;
    run->pl.steps_per_unit = run->sp.steps_per_unit;
    KMU_TRY(seg_buffers(ctx, run->pl, run->sp, total_bases, own_buffer, &run->b));
    const uint64_t nsteps = std::max<uint64_t>(1, flat_wave_steps(total_bases));
    return flat_novalid(ctx, ds, total_bases, c->p.kmer_size, nsteps * 64 + 64, "cnt.novalid", &run->novalid);
}
// level 1 for the wave steps that (with their 32-base halo) lie inside the first `bases_ready` bases of the stream and have not
// been through it (seg_round): every unit takes its slice of them
static int seg_level1(kmu_counter *c, SegRun *run, uint64_t bases_ready) {
    kmu_ctx *ctx = c->ctx;
    if (run->l1_done) return KMU_OK;
    // an arrival of less than a few tiles per wave waits for the next one (KMU_COUNT_SEG_ROUND_MIN: tests); the last launch is made in any case
    const char *mn = getenv("KMU_COUNT_SEG_ROUND_MIN");
    const SegRound r = seg_round(run->total_bases, bases_ready, run->steps_done, run->sp.units1, mn ? (uint64_t) atoi(mn) : 64u);
    if (r.launch) {
        PartPlan pl = run->pl;
        pl.steps_per_unit = (uint32_t) ((r.n_new + run->sp.units1 - 1) / run->sp.units1);
        KMU_TRY(launch(ctx, "k_part_scatter1", k_part_scatter1, dim3(run->sp.units1), dim3(SCATTER_THREADS), seg_lds_bytes(plan_bins1(pl)),
                       run->ds.bases, run->ds.offsets, run->ds.n_seq, c->p.kmer_size, pl, (uint64_t *) run->b.A, SegPlan1{run->sp.cap1,
                       run->steps_done, run->steps_done + r.n_new, (uint32_t *) run->b.ovf, run->d_err, (uint32_t *) run->b.state, run->sp.sets,
                       (const uint16_t *) run->novalid}));
    }
    run->steps_done += r.n_new;
    if (r.last) {
        run->l1_done = true;
        KMU_TRY(seg_tails(ctx, run->pl, run->sp, run->b));
    }
    return KMU_OK;
}
// the rest of level 1, then the tail
static int seg_finish(kmu_counter *c, SegRun *run, int *taken) {
    KMU_TRY(seg_level1(c, run, run->total_bases));
    return seg_level2_build(c, run->pl, run->sp, run->b, run->d_err, taken);
}

// the single-pass partition for an ARRAY of canonical k-mers (what the owner of a key range receives in the OCCURRENCES
// route of a distributed add): level 1 cuts the array into chunks, sets of shared streams, no histograms
// recs != nullptr: the input is n_rec super-k-mer records holding n k-mers (kmu_smer.h) instead of an array of n k-mers
int seg_partitioned_add_kmers(kmu_counter *c, const uint64_t *d_kmers, uint64_t n, const PartPlan &pl, uint32_t *d_err, int *taken,
                              const void *recs, uint64_t n_rec) {
    kmu_ctx *ctx = c->ctx;
    *taken = 0;
    const uint32_t bins1 = plan_bins1(pl);
    const SegPlan sp = seg_plan_array((uint32_t) ctx->num_cus, n, bins1, pl.n2, seg_cap_share());
    SegBufs b;
    void *b0;
    KMU_TRY(seg_buffers(ctx, pl, sp, n, false, &b));
    KMU_TRY(dev_buf(ctx, "arr.bounds0", 16, &b0));
    KMU_TRY(launch(ctx, nullptr, k_fill_linear, dim3(1), dim3(256), 0, (uint64_t *) b0, (uint64_t) 2, n));
    const ArrPlan ap1{plan_digit1(pl), bins1, 1u, sp.units1, 0u, 0u, 0u, sp.sets};
    if (recs) {
        KMU_TRY(launch(ctx, "k_smer_scatter1", k_smer_scatter1, dim3(sp.units1), dim3(SCATTER_THREADS), seg_lds_bytes(bins1), (const uint32_t *) recs,
                       n_rec, c->p.kmer_size, ap1, (uint64_t *) b.A, sp.cap1, (uint32_t *) b.ovf, (uint32_t *) b.state));
    } else {
        KMU_TRY(launch(ctx, "k_arr_scatter", k_arr_scatter_seg<IT_KEY_TO_HASH, false>, dim3(sp.units1), dim3(SCATTER_THREADS), seg_lds_bytes(bins1),
                       d_kmers, (const uint64_t *) b0, ap1, (uint64_t *) b.A, sp.cap1, (uint32_t *) b.ovf, (uint32_t *) b.state,
                       (const uint32_t *) nullptr));
    }
    KMU_TRY(seg_tails(ctx, pl, sp, b));
    return seg_level2_build(c, pl, sp, b, d_err, taken);
}

// ---- the exact levels ----------------------------------------------------------------------------------------------------
// the units of the exact level 1 over reads and of the censuses: up to eight workgroups per CU
static void plan_units(const kmu_ctx *ctx, uint64_t total_bases, PartPlan *pl) {
    const UnitSplit us = unit_split(flat_wave_steps(total_bases), (uint64_t) ctx->num_cus * 8);
    pl->units1 = us.units;
    pl->steps_per_unit = us.steps_per_unit;
}
// The exact level 1 over reads, first half: the per-unit histogram of the level-1 digit of op->pl (its units set: plan_units;
// it validates the bases and takes the key sample `sa` asks for), the scans.  op carries the buffers to reads_scatter_exact.
static int reads_census(kmu_counter *c, const DevSeqs &ds, uint32_t *d_err, const SampleArgs &sa, OwnerPlan *op) {
    kmu_ctx *ctx = c->ctx;
    const PartPlan &pl = op->pl;
    const uint32_t bins1 = plan_bins1(pl);
    KMU_TRY(dev_buf(ctx, "cnt.hist1", (size_t) pl.units1 * bins1 * 4, &op->hist1));
    KMU_TRY(dev_buf(ctx, "cnt.offs1", (size_t) pl.units1 * bins1 * 8, &op->offs1));
    KMU_TRY(dev_buf(ctx, "cnt.tot1", (size_t) bins1 * 8, &op->tot1));
    KMU_TRY(dev_buf(ctx, "cnt.binstart1", (size_t) (bins1 + 1) * 8, &op->binstart1));
    // (the two words behind the histogram are the sample's counter: a table's digits touch only lh[0 .. bins1))
    const size_t lds = ((size_t) bins1 + 2) * 4 + (sa.list ? 16 + (size_t) SAMPLE_LDS * 8 : 0);
    KMU_TRY(launch(ctx, "k_part_hist1", k_part_hist1, dim3(pl.units1), dim3(256), lds, ds.bases, ds.offsets, ds.n_seq, c->p.kmer_size, pl,
                   (uint32_t *) op->hist1, d_err, sa));
    {
        KernelTimer tm(ctx, "k_part_scan1");
        KMU_TRY(launch(ctx, nullptr, k_part_scan1a, dim3(bins1), dim3(256), 0, (const uint32_t *) op->hist1, pl, (uint64_t *) op->offs1,
                       (uint64_t *) op->tot1));
        KMU_TRY(launch(ctx, nullptr, k_part_scan1b, dim3(1), dim3(256), 0, (const uint64_t *) op->tot1, pl, (uint64_t *) op->binstart1));
    }
    return KMU_OK;
}
// second half: every unit scatters its k-mers into its private ranges of `out` (bin b at op.binstart1[b])
static int reads_scatter_exact(kmu_counter *c, const DevSeqs &ds, const OwnerPlan &op, uint64_t *out) {
    kmu_ctx *ctx = c->ctx;
    KMU_TRY(scatter_attrs(ctx));
    KMU_TRY(launch(ctx, "k_part_scatter1", k_part_scatter1_exact, dim3(op.pl.units1), dim3(SCATTER_THREADS), scatter_lds_bytes(plan_bins1(op.pl)),
                   ds.bases, ds.offsets, ds.n_seq, c->p.kmer_size, op.pl, (const uint64_t *) op.offs1, (const uint64_t *) op.binstart1, out));
    return KMU_OK;
}

// One exact level over an array: the ap.nparts partitions of `in` (their bounds in `bounds`) into ap.bins bins each -- histogram,
// scans, scatter into `out`; *outbounds: the bounds of the nparts * bins partitions of `out`.  `it` is the scatter's form and
// names what comes in and what goes out: IT_KEY (keys, keys), IT_KEY_TO_HASH (keys, khash(key)), IT_HASH (khash, khash).
// The scratch buffers go by the caller's names ("arr.*" and "cnt.*" stay apart: OwnerPlan points into "cnt.*" across calls).
struct ArrScratch { const char *tot, *hist, *offs, *bounds; };
static int arr_level_exact(kmu_ctx *ctx, int it, const ArrPlan &ap, const ArrScratch &names, const uint64_t *in, const uint64_t *bounds,
                           uint64_t *out, const uint64_t **outbounds) {
    KMU_TRY(scatter_attrs(ctx));
    const uint32_t units = ap.nparts * ap.chunks;
    const size_t n_out = (size_t) ap.nparts * ap.bins;
    uint64_t *outb, *offs, *tot;
    uint32_t *hist;
    KMU_TRY(dev_array(ctx, names.tot, n_out, &tot));
    KMU_TRY(dev_array(ctx, names.hist, (size_t) units * ap.bins, &hist));
    KMU_TRY(dev_array(ctx, names.offs, (size_t) units * ap.bins, &offs));
    KMU_TRY(dev_array(ctx, names.bounds, n_out + 1, &outb));
    KMU_TRY(launch(ctx, "k_arr_hist", it == IT_HASH ? k_arr_hist<IT_HASH> : k_arr_hist<IT_KEY>, dim3(units), dim3(256), ap.bins * 4, in, bounds, ap,
                   hist));
    {
        KernelTimer tm(ctx, "k_arr_scan");
        const uint32_t T = std::min<uint32_t>(256u, 1u << (31 - __builtin_clz(std::max<uint32_t>(1u, ap.chunks)))), per_wg = 256u / T;
        KMU_TRY(launch(ctx, nullptr, k_arr_scan_a, dim3(ap.nparts * ((ap.bins + per_wg - 1) / per_wg)), dim3(256), 0, hist, ap, T, offs, tot));
        KMU_TRY(launch(ctx, nullptr, k_arr_scan_b, dim3(ap.nparts), dim3(256), 0, tot, bounds, ap, outb));
    }
    const auto scatter = it == IT_HASH ? k_arr_scatter_exact<IT_HASH> : it == IT_KEY ? k_arr_scatter_exact<IT_KEY> : k_arr_scatter_exact<IT_KEY_TO_HASH>;
    KMU_TRY(launch(ctx, "k_arr_scatter", scatter, dim3(units), dim3(SCATTER_THREADS), scatter_lds_bytes(ap.bins), in, bounds, ap, offs, outb, out));
    *outbounds = outb;
    return KMU_OK;
}
// the radix-partitioned build over device-resident ASCII reads
int partitioned_add(kmu_counter *c, const DevSeqs &ds, uint64_t total_bases, uint32_t *d_err) {
    kmu_ctx *ctx = c->ctx;
    OwnerPlan l1; // (the plan of level 1 and the buffers of its census)
    PartPlan &pl = l1.pl;
    if (!part_plan_for(c, &pl)) return fail(ctx, KMU_E_UNSUPPORTED, "table too large for the two-level partitioned build");
    const uint32_t bins1 = plan_bins1(pl);
    const bool two = pl.b1 != 0;
    // the single-pass partition first, BEFORE the exact route takes its buffers: both use "cnt.partA" / "cnt.partB" with different
    // sizes, and a buffer that grows is freed and allocated anew (pointers taken earlier would dangle)
    if (two && !c->no_seg && seg_partition_wanted(total_bases)) {
        SegRun run;
        int taken = 0;
        KMU_TRY(seg_begin(c, ds, total_bases, pl, d_err, &run));
        KMU_TRY(seg_finish(c, &run, &taken));
        if (taken) return KMU_OK; // (else the spill list overflowed -- very skewed k-mers -- and nothing was touched: the exact route)
    }
    // (total_bases == 0 used to divide by zero here and is now one unit of one step; no caller brings it this far: no change of behaviour)
    plan_units(ctx, total_bases, &pl);
    pl.chunks2 = two ? std::max<uint32_t>(1u, 16384u / bins1) : 1u;
    uint64_t *B, *A;
    KMU_TRY(dev_array(ctx, "cnt.partA", total_bases + 8, &A));
    KMU_TRY(reads_census(c, ds, d_err, SampleArgs{nullptr, nullptr, 0u, 0u}, &l1));
    KMU_TRY(reads_scatter_exact(c, ds, l1, A));
    if (!two) return launch_build<IT_HASH>(c, A, (const uint64_t *) l1.binstart1, d_err);
    const uint64_t *leafstart;
    const ArrPlan ap{plan_digit2(pl), pl.n2, bins1, pl.chunks2, 0u, 0u, 0u, 0u};
    KMU_TRY(dev_array(ctx, "cnt.partB", total_bases + 8, &B));
    KMU_TRY(arr_level_exact(ctx, IT_HASH, ap, ArrScratch{"cnt.tot2", "cnt.hist2", "cnt.offs2", "cnt.leafstart"}, A,
                            (const uint64_t *) l1.binstart1, B, &leafstart));
    return launch_build<IT_HASH>(c, B, leafstart, d_err);
}

// Partition a device array of u64 keys by the digits of `pl` into its 2^b1 * n2 leaves (exact levels).  Returns the partitioned
// copy and the leaf bounds (both in context scratch buffers, valid until the next partition call).
// hashed_out: the output items are khash(key) instead of the keys (what the region builds of IT_HASH take).
static int partition_by_plan(kmu_ctx *ctx, const uint64_t *in, uint64_t n, const PartPlan &pl, const uint64_t **items_out,
                             const uint64_t **bounds_out, bool hashed_out) {
    static const ArrScratch names[2] = {{"arr.tot0", "arr.hist0", "arr.offs0", "arr.bounds1"}, {"arr.tot1", "arr.hist1", "arr.offs1", "arr.bounds2"}};
    void *b0;
    KMU_TRY(dev_buf(ctx, "arr.bounds0", 16, &b0));
    uint64_t h0[2] = {0, n};
    KMU_HIP(ctx, hipMemcpyAsync(b0, h0, 16, hipMemcpyHostToDevice, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream)); // h0 lives on the stack
    const uint64_t *bounds = (const uint64_t *) b0;
    const uint64_t *items = in;
    uint32_t nparts = 1;
    int it = hashed_out ? IT_KEY_TO_HASH : IT_KEY; // (the first executed level still reads keys)
    const int nlevels = pl.b1 ? 2 : 1;
    for (int level = 0; level < nlevels; level++) {
        const bool by_group = nlevels == 2 && level == 0;
        const uint32_t bins = by_group ? 1u << pl.b1 : pl.n2;
        if (bins <= 1) continue;
        const uint32_t chunks = level == 0 ? (uint32_t) std::min<uint64_t>(std::max<uint64_t>(1, n / 65536), 16384)
                                           : std::max<uint32_t>(1u, 16384u / nparts);
        const ArrPlan ap{by_group ? plan_digit1(pl) : plan_digit2(pl), bins, nparts, chunks, 0u, 0u, 0u, 0u};
        uint64_t *out;
        KMU_TRY(dev_array(ctx, level == 0 ? "cnt.partA" : "cnt.partB", n + 8, &out));
        KMU_TRY(arr_level_exact(ctx, it, ap, names[level], items, bounds, out, &bounds));
        items = out;
        nparts *= bins;
        if (hashed_out) it = IT_HASH;
    }
    *items_out = items;
    *bounds_out = bounds;
    return KMU_OK;
}
// Partition a device array of u64 keys by the top `region_bits` bits of khash(key) into 2^region_bits leaves (<= 22 bits: two
// 11-bit passes): the sketch path's partition of pre-hashed values (sketch_all_hashed, kmu_sketch.hip)
int partition_u64(kmu_ctx *ctx, const uint64_t *in, uint64_t n, int region_bits, const uint64_t **items_out,
                  const uint64_t **bounds_out, bool hashed_out) {
    if (region_bits > 22) return fail(ctx, KMU_E_UNSUPPORTED, "too many partitions (2^%d)", region_bits);
    PartPlan pl;
    memset(&pl, 0, sizeof pl);
    region_split(region_bits, &pl.b1, &pl.n2);
    return partition_by_plan(ctx, in, n, pl, items_out, bounds_out, hashed_out);
}
// big batches of explicit canonical k-mers (device arrays): partition by region, then the LDS build
int partitioned_add_kmers(kmu_counter *c, const uint64_t *d_kmers, uint64_t n, uint32_t *d_err) {
    kmu_ctx *ctx = c->ctx;
    PartPlan pl;
    if (!part_plan_for(c, &pl)) return fail(ctx, KMU_E_UNSUPPORTED, "table too large for the two-level partitioned build");
    // (the single-pass attempt first, then the exact levels take "cnt.partA" / "cnt.partB" anew: see partitioned_add)
    if (!c->no_seg && pl.b1 && seg_partition_wanted(n)) {
        int taken = 0;
        KMU_TRY(seg_partitioned_add_kmers(c, d_kmers, n, pl, d_err, &taken));
        if (taken) return KMU_OK;
    }
    const uint64_t *items, *bounds;
    // (a table of a single region is not partitioned at all: the items stay keys)
    const bool hashed = plan_regions(pl) > 1;
    KMU_TRY(partition_by_plan(ctx, d_kmers, n, pl, &items, &bounds, hashed));
    if (hashed) return launch_build<IT_HASH>(c, items, bounds, d_err);
    return launch_build<IT_KEY>(c, items, bounds, d_err);
}

// canonical k-mers of the reads, grouped by owner rank (the exact level 1 with digit = owner), in two halves, so that a
// distributed add can look at the duplication sample between them
int owner_census(kmu_counter *c, const DevSeqs &ds, uint64_t total_bases, uint32_t n_parts, uint32_t *d_err, OwnerPlan *op,
                 const SampleArgs &sa) {
    if (n_parts == 0 || n_parts > 2048) return fail(c->ctx, KMU_E_BAD_ARG, "n_parts must be in 1..2048");
    memset(&op->pl, 0, sizeof op->pl);
    op->pl.owner_parts = n_parts;
    op->pl.owner_w32 = kmer_val_bytes(c->p.kmer_type) == 4;
    plan_units(c->ctx, total_bases, &op->pl);
    return reads_census(c, ds, d_err, sa, op);
}
int owner_scatter(kmu_counter *c, const DevSeqs &ds, uint64_t total_bases, const OwnerPlan &op, uint64_t **dev_out) {
    uint64_t *out;
    KMU_TRY(dev_array(c->ctx, "cnt.partB", total_bases + 8, &out));
    *dev_out = out;
    return reads_scatter_exact(c, ds, op, *dev_out);
}
// distinct keys of a device list of n sampled k-mers (scratch: "cnt.sample_tab"; d_word: a device word for the count)
int sample_distinct(kmu_ctx *ctx, const uint64_t *d_list, uint32_t n, uint32_t *d_word, uint32_t *distinct_out) {
    *distinct_out = 0;
    if (!n) return KMU_OK;
    void *stab;
    uint32_t tbits = 10;
    while ((1ull << tbits) < 2ull * n) tbits++;
    KMU_TRY(dev_buf(ctx, "cnt.sample_tab", ((size_t) 8 << tbits) + 64, &stab));
    KMU_HIP(ctx, hipMemsetAsync(stab, 0xFF, (size_t) 8 << tbits, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(d_word, 0, 4, ctx->stream));
    KMU_TRY(launch(ctx, "k_sample_distinct", k_sample_distinct, dim3(grid_for(ctx, n, 256)), dim3(256), 0, d_list, n, (uint64_t *) stab,
                   (uint32_t) ((1u << tbits) - 1u), d_word));
    KMU_HIP(ctx, hipMemcpyAsync(distinct_out, d_word, 4, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMU_OK;
}
// occurrences / distinct of the k-mers of a batch of reads, from the key sample of a census pass (0: no estimate)
int sample_ratio(kmu_counter *c, const DevSeqs &ds, uint64_t total_bases, uint32_t *d_err, double *ratio_out) {
    kmu_ctx *ctx = c->ctx;
    *ratio_out = 0.0;
    uint64_t *slist;
    void *sn;
    const uint64_t units = unit_split(flat_wave_steps(total_bases), (uint64_t) ctx->num_cus * 8).asked; // (the shift goes by the count before re-rounding)
    const uint64_t kmers_per_unit = (total_bases + units - 1) / units;
    uint32_t shift = 0; // ~1024 sampled k-mers per workgroup (its LDS list holds 4096)
    while (shift < 24 && (kmers_per_unit >> shift) > 1024) shift++;
    const uint32_t cap = (uint32_t) std::min<uint64_t>(units * SAMPLE_LDS, 1u << 26);
    KMU_TRY(dev_array(ctx, "cnt.sample", (size_t) cap + 8, &slist));
    KMU_TRY(dev_buf(ctx, "cnt.sample_n", 64, &sn));
    KMU_HIP(ctx, hipMemsetAsync(sn, 0, 64, ctx->stream));
    OwnerPlan op;
    KMU_TRY(owner_census(c, ds, total_bases, 1, d_err, &op, SampleArgs{slist, (uint32_t *) sn, cap, shift}));
    uint32_t h_sn[2] = {0, 0};
    KMU_HIP(ctx, hipMemcpyAsync(h_sn, sn, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n_s = std::min(h_sn[0], cap);
    if (!n_s || h_sn[1]) return KMU_OK; // nothing sampled, or a truncated sample: no estimate
    uint32_t d_s = 0;
    KMU_TRY(sample_distinct(ctx, slist, n_s, (uint32_t *) sn + 2, &d_s));
    if (d_s) *ratio_out = (double) n_s / (double) d_s;
    return KMU_OK;
}

// kmu_sketch_count on host buffers: the count's level-1 partition runs chunk by chunk under the upload (the single-pass
// partition needs no histogram of the whole batch).  count_chunked_begin returns *on = 0 when that route does not apply
// (a distributed counter, a small batch, a one-level table): the caller then adds the reads in one go at the end.  The handle is a SegRun.
int count_chunked_begin(kmu_counter *c, DevSeqs &all, const uint64_t *host_offsets, uint32_t *d_err, void **handle, int *on) {
    *on = 0;
    *handle = nullptr;
    if (c->dist || all.n_seq == 0) return KMU_OK;
    uint64_t total_bases = 0;
    KMU_TRY(flat_stream_extent(c->ctx, host_offsets, all.n_seq, KMU_MEM_HOST, all, &total_bases));
    KMU_TRY(table_alloc_for(c, nullptr, 0, d_err)); // (the reads are not on the device yet: a table by the hint)
    PartPlan pl;
    const bool partitioned = partitioned_batch_wanted(c, total_bases);
    if (!partitioned || !part_plan_for(c, &pl) || !pl.b1 || !seg_partition_wanted(total_bases)) return KMU_OK;
    SegRun *run = new SegRun();
    const int rc = seg_begin(c, all, total_bases, pl, d_err, run, true);
    if (rc != KMU_OK) { delete run; return rc; }
    *handle = run;
    *on = 1;
    return KMU_OK;
}
int count_chunked_level1(kmu_counter *c, void *handle, uint64_t bases_ready) { return seg_level1(c, (SegRun *) handle, bases_ready); }
int count_chunked_finish(kmu_counter *c, void *handle) {
    SegRun *run = (SegRun *) handle;
    int taken = 0;
    int rc = seg_finish(c, run, &taken);
    if (rc == KMU_OK && !taken) { // the spill list overflowed: the exact route (not a second attempt on the same k-mers)
        c->no_seg = true;
        rc = local_add(c, run->ds, run->total_bases, run->d_err);
        c->no_seg = false;
    }
    delete run;
    return rc;
}
void count_chunked_abort(void *handle) { delete (SegRun *) handle; }

} // namespace kmu

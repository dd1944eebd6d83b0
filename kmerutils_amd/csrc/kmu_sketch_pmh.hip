// kmu_sketch_pmh.hip -- the host side of ProbMinHash3a / bottom-k: which kernels a batch takes (routes chosen per call from the
// batch's shape), their launches and scratch buffers, and the long-sequence detour of the per-sequence path.
// The kernels are in kmu_pmh_*.hip, one file per route (declarations: kmu_sketch_kernels.h; shared device steps: kmu_pmh_steps.h).
#include <algorithm>
#include <cmath>

#include "kmu_sketch_host.hpp"
#include "kmu_sketch_kernels.h"

using namespace kmu;

static int atoi_or(const char *s, int dflt) { return s ? atoi(s) : dflt; }

// ProbMinHash3a of whole DNA sequences with k <= 8 (Kmer32bit) and a closure that is injective on the (canonical) k-mer:
// the histogram route of k_sketch_smallk.  KMU_PMH_SMALLK=0 keeps the general kernels (diagnostics, A/B).
static bool smallk_route(const kmu_sketch_params *p, int hashed_bytes, bool partial, bool blocks) {
    if (p->algo != KMU_ALGO_PROB3A || p->kmer_type != KMU_KMER32BIT || p->kmer_size > 8 || hashed_bytes || partial || blocks ||
        p->block_size != 0 || p->sketch_size > 512)
        return false;
    switch (p->fhash) {
    case KMU_FHASH_IDENTITY_RAW: case KMU_FHASH_VALUE_MASKED: case KMU_FHASH_CANON_RAW: case KMU_FHASH_CANON_INVHASH:
    case KMU_FHASH_INVHASH_RAW: case KMU_FHASH_CANON_VALUE: break;
    default: return false; // (ntHash is not injective in principle)
    }
    return atoi_or(getenv("KMU_PMH_SMALLK"), 1) != 0;
}

// The routes of a ProbMinHash3a / bottom-k call and the kernels they launch:
//  SMALLK    k <= 8: k_sketch_smallk, with lists + k_pmh_points
//  SHORT     whole unpacked reads of at most 256 k-mers: k_multiset_short + k_pmh_points_short
//  UQ        whole unpacked reads: k_multiset_uq (two shapes), k_multiset_long for the longer ones, the list-emitting k_sketch_pmh3a for
//            what that one hands back, k_pmh_points
//  LISTS     whole reads, packed (or KMU_PMH_PLAIN=0): the list-emitting k_sketch_pmh3a + k_pmh_points
//  ONE_PASS  whole unpacked reads without lists: PLAIN k_sketch_pmh3a, the reads it hands back through the general one
//  GENERAL   the general k_sketch_pmh3a: bottom-k, AA / pre-hashed, packed, partial rows, blocks
enum class PmhRoute { SMALLK, SHORT, UQ, LISTS, ONE_PASS, GENERAL };
struct PmhPlan {
    PmhRoute route = PmhRoute::GENERAL;
    bool lists = false;        // (key, weight) lists in HBM: SHORT, UQ, LISTS, and SMALLK when they fit
    uint64_t list_bases = 0;   // their capacity: the bases of the batch
    uint32_t pts_long = 32768; // KMU_PMH_PTS_LONG, as given (launch_points clamps it).  (bench: the device leg is the same with or
                               //  without; the host leg's chunks gain 1.3 ms of 128; 16 384: +0.4 ms on the device leg, 8 192: +2)
    int cus = 0;               // CUs the kernels spread over (KMU_PMH_RESERVE_CUS)
};

// the (key, weight) lists of the two-kernel routes, one entry per base of the batch.  8 bytes per key: the same scratch the
// count build uses for its first partition level ("cnt.partA"); a context never runs the two at the same time, and at
// 4.4 Gbases per GPU a second copy would not fit next to the count table and the exchange buffers
static int alloc_lists(kmu_ctx *ctx, SketchArgs &a, uint64_t bases) {
    void *ln;
    KMU_TRY(dev_array(ctx, "cnt.partA", bases + 8, &a.lst_keys));
    KMU_TRY(dev_array(ctx, "pmh.lst_w", bases + 16, &a.lst_w));
    KMU_TRY(dev_buf(ctx, "pmh.lst_n", (size_t) a.n_seq * 8 + 64, &ln));
    a.lst_n = (uint32_t *) ln;
    a.lst_nu = a.lst_n + a.n_seq;
    KMU_HIP(ctx, hipMemsetAsync(a.lst_nu, 0, (size_t) a.n_seq * 4, ctx->stream));
    return KMU_OK;
}

// The one route decision of a call; the sketch route's KMU_PMH_* switches are read here, once each.
static int pmh_route(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const PmhInputs &in, PmhPlan *plan) {
    const int split_mode = atoi_or(getenv("KMU_PMH_SPLIT"), -1);     // 0 / 1: never / always the lists
    const bool plain_on = atoi_or(getenv("KMU_PMH_PLAIN"), 1) != 0; // 0: never the PLAIN instantiation (diagnostics)
    const bool short_on = atoi_or(getenv("KMU_PMH_SHORT"), 1) != 0; // 0: short reads through k_multiset_uq (A/B)
    plan->pts_long = (uint32_t) std::max(0, atoi_or(getenv("KMU_PMH_PTS_LONG"), 32768));
    const int cus = ctx->num_cus; // less the CUs left to concurrent work (RCCL kernels of an exchange in flight)
    plan->cus = std::max(cus / 2, cus - std::max(0, atoi_or(getenv("KMU_PMH_RESERVE_CUS"), 0)));
    const bool smallk = smallk_route(p, in.hashed_bytes, in.part_h != nullptr, in.d_block_rows != nullptr);
    // whole sequences of bases to signature rows
    const bool whole = p->algo != KMU_ALGO_BOTTOMK && !kmer_is_aa(p->kmer_type) && !in.hashed_bytes && !in.part_h &&
                       !in.d_block_rows && p->block_size == 0;
    // SMALLK: the distinct (key, weight) pairs go to k_pmh_points through the lists unless that memory is not to be had: then
    // the histogram kernel makes the points itself.
    // Big batches of whole DNA sequences go through two kernels: the multiset kernel leaves the (key, weight) pairs of
    // every read in HBM, k_pmh_points (one wave per read, no workgroup barrier, 5 waves per SIMD) generates the points.
    // ONT workload: 53.3 + 21.2 ms against 88.7 ms in one kernel, for 12 bytes of scratch per base.  One wave per read
    // has a tail: the longest read keeps its wave busy while the others have run out of reads.  The route is taken
    // when the gain (16 % of the single kernel's time) exceeds the expected overhang of that read; figures of an MI355X
    // (a wave of k_pmh_points does 4.0e4 k-mers per ms, the single kernel 4.9e7 per ms with 256 CUs).
    bool lists = (size_t) 4 * (2 * (size_t) p->sketch_size + PTS_WAVE_WORDS) * 8 + WINV_LUT * 8 <= 150 * 1024 && // four waves' arrays fit one workgroup
                 split_mode != 0 && (smallk || (whole && !in.skip_longer && (split_mode == 1 || in.len_stats)));
    const bool judge = !smallk && split_mode != 1; // (KMU_PMH_SPLIT=1: the two-kernel route whatever it costs)
    if (lists) {
        uint64_t &total = plan->list_bases; // the lists' capacity: bases in the batch
        if (in.len_stats) total = in.len_stats[1];
        else if (!ds.h_offsets.empty()) total = ds.h_offsets[ds.n_seq] - ds.h_offsets[0];
        else {
            uint64_t ends[2] = {0, 0};
            KMU_TRY(read_back(ctx, {{&ends[0], ds.offsets}, {&ends[1], ds.offsets + ds.n_seq}}));
            total = ends[1] - ends[0];
        }
        if (judge) {
            const uint64_t longest = in.len_stats[0];
            const double cu_share = (double) ctx->num_cus / 256.0;
            // (a wave of k_pmh_points does 4.0e4 k-mers per ms; a read beyond KMU_PMH_PTS_LONG is taken by four)
            const double wave_rate = plan->pts_long && longest > plan->pts_long ? 1.6e5 : 4.0e4;
            const double t_ideal = (double) total / (2.35e8 * cu_share), t_tail = (double) longest / wave_rate; // ms
            const double overhang = t_tail >= t_ideal ? t_tail - 0.5 * t_ideal : t_tail * t_tail / (2.0 * t_ideal);
            // (r02: with the reads that fit a workgroup's registers on k_multiset_uq the two-kernel route takes 53 ms where the
            //  single kernel takes 87 on the ONT workload: 39 % of the single kernel's time, 16 % before)
            // (r03: 49.8 ms, 43 %; the points kernel 18.5 ms for 4.36 G k-mers)
            const double gain = 0.43 * (double) total / (4.9e7 * cu_share);
            if (gain <= overhang + 0.02) lists = false; // (0.02 ms: the second launch)
        }
        if (lists && (smallk || judge)) { // the lists would crowd out what comes after this call: one kernel, no lists
            const size_t need_k = total * 8 + 64, need_w = total * 4 + 64;
            size_t grow = 0, free_b = 0, total_b = 0;
            if (ctx->bufs["cnt.partA"].bytes < need_k) grow += need_k + need_k / 8;
            if (ctx->bufs["pmh.lst_w"].bytes < need_w) grow += need_w + need_w / 8;
            if (grow && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < grow + total_b / 8) lists = false;
        }
    }
    plan->lists = lists;
    const bool plain = whole && !ds.packed && plain_on;
    // (every read of the batch with at most 256 k-mers: one wave per read)
    const bool short_reads = in.len_stats && in.len_stats[0] < (uint64_t) SHORT_KEYS + (uint64_t) p->kmer_size && short_on;
    plan->route = smallk         ? PmhRoute::SMALLK
                  : lists && plain ? (short_reads ? PmhRoute::SHORT : PmhRoute::UQ)
                  : lists          ? PmhRoute::LISTS
                  : plain          ? PmhRoute::ONE_PASS
                                   : PmhRoute::GENERAL;
    return KMU_OK;
}

static int alloc_queue(kmu_ctx *ctx, SketchArgs &a) {
    void *q;
    KMU_TRY(dev_buf(ctx, "queue", 256, &q)); // u32 words: [0] read cursor, [48] queue2, [56] count of long / redo reads
    KMU_HIP(ctx, hipMemsetAsync(q, 0, 256, ctx->stream));
    a.queue = (uint32_t *) q;
    return KMU_OK;
}

// k_pmh_points over the lists of a.n_seq reads; reads with more than pts_long list entries (KMU_PMH_PTS_LONG, default 32 768;
// 0: none) are listed first (k_pts_long_list) and taken by whole workgroups
static int launch_points(kmu_ctx *ctx, SketchArgs a, int cus, uint32_t thr) {
    void (*const kpts)(SketchArgs) = a.sig_bytes == 4 ? k_pmh_points<true> : k_pmh_points<false>;
    const size_t lds2 = (size_t) 4 * (2 * (size_t) a.m + PTS_WAVE_WORDS) * 8 + WINV_LUT * 8;
    if (lds2 > 64 * 1024)
        KMU_HIP(ctx, hipFuncSetAttribute((const void *) kpts, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(8, (160 * 1024) / lds2));
    const int grid2 = (int) std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t) a.n_seq + 3) / 4, (uint64_t) cus * per_cu)); // (cus: see KMU_PMH_RESERVE_CUS)
    a.pts_long = nullptr;
    a.pts_long_t = thr;
    if (thr && a.n_seq) {
        if (thr < 1024u) a.pts_long_t = thr = 1024u; // (a workgroup's four waves all need chunks of their own)
        KMU_TRY(dev_array(ctx, "pts.long", (size_t) a.n_seq + 2 + 16, &a.pts_long));
        KMU_HIP(ctx, hipMemsetAsync(a.pts_long, 0, 8, ctx->stream));
        KMU_TRY(launch(ctx, nullptr, k_pts_long_list, dim3((a.n_seq + 255) / 256), dim3(256), 0, a.lst_n, a.n_seq, thr, a.pts_long));
    }
    // the a-priori q_max bound of pts_one_read.  KMU_PMH_TAU_C (read once per context): unset = PTS_TAU_C; 0 / off = no bound;
    // a negative c makes nearly every read fail the bound and start over (tests of that path)
    if (!ctx->pmh_tau_read) {
        const char *e = getenv("KMU_PMH_TAU_C");
        ctx->pmh_tau_c = !e ? PTS_TAU_C : (!strcmp(e, "off") ? 0.0 : atof(e));
        ctx->pmh_tau_read = true;
    }
    const bool fresh = !ctx->bufs.count("pmh.tau_redo");
    void *tr;
    KMU_TRY(dev_buf(ctx, "pmh.tau_redo", 4, &tr));
    if (fresh) KMU_HIP(ctx, hipMemsetAsync(tr, 0, 4, ctx->stream)); // (counts until kmu_profile_reset)
    a.tau_redo = (uint32_t *) tr;
    a.tau_num = (double) a.m * (std::log((double) a.m) + ctx->pmh_tau_c);
    a.tau_min_n = ctx->pmh_tau_c != 0.0 && a.tau_num > 0.0 ? (uint32_t) std::min(a.tau_num, 4.0e9) : 0xFFFFFFFFu;
    a.tau_hold = PTS_TAU_HOLD;
    return launch(ctx, "k_pmh_points", kpts, dim3(grid2), dim3(256), lds2, a);
}

typedef void (*sketch_kernel_t)(SketchArgs);

static int launch_main(kmu_ctx *ctx, const SketchArgs &a, sketch_kernel_t kern, int grid, size_t lds, const char *name) {
    return launch(ctx, name, kern, dim3(grid), dim3(1024), lds, a);
}

static int launch_smallk(kmu_ctx *ctx, SketchArgs a, const PmhPlan &plan) {
    // (Round 4, measured and not kept: the first point of every one of the 4^k possible keys from a table made once per call -- no
    //  generator in pass 1 -- but 4e9 gathers of 16 bytes out of a 1 MB table are 4e9 lines from L2: k_pmh_points 26.1 against 18.9 ms
    //  on config 3; 16-bit lower bounds of the samples in LDS in front of the gather: 52 ms.)
    const sketch_kernel_t kern = plan.lists ? k_sketch_smallk<true> : k_sketch_smallk<false>;
    // LDS: histogram | slot minima (only when the kernel makes the points itself) | list of u16 indices | staged words
    const size_t lds_fixed = (size_t) SMALLK_WORDS * 4 + (plan.lists ? 0 : (size_t) 16 * a.m) + ((size_t) SMALLK_TILE + 2) * 4 + 64;
    a.cap = (uint32_t) ((160 * 1024 - lds_fixed) / 2) & ~2047u;
    if (a.cap > 32768u) a.cap = 32768u;
    const size_t lds = lds_fixed + (size_t) a.cap * 2;
    KMU_HIP(ctx, hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    KMU_TRY(alloc_queue(ctx, a));
    a.queue2 = a.queue + 48;
    const int grid = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) a.n_seq, (uint64_t) plan.cus));
    KMU_TRY(launch_main(ctx, a, kern, grid, lds, "k_sketch_smallk"));
    if (plan.lists) KMU_TRY(launch_points(ctx, a, plan.cus, plan.pts_long));
    return KMU_OK;
}

// The general kernel's launch shape, shared by every route but SMALLK
struct PmhShape {
    size_t lds;     // what one workgroup takes
    uint64_t slots; // workgroups resident at once on the CUs in use
    int grid;
};

// LDS budget (tile_words, cap, part_target, tile_shift) of `kern`, the read queue, the grid and the scratch sized by it;
// plain: the routes whose reads may be handed back to the general instantiation (redo list)
static int pmh_shape(kmu_ctx *ctx, const kmu_sketch_params *p, SketchArgs &a, sketch_kernel_t kern, bool plain, int cus, PmhShape *g) {
    const bool bottomk = p->algo == KMU_ALGO_BOTTOMK, aa = kmer_is_aa(p->kmer_type) || a.hashed_bytes != 0;
    a.bk_shift = (a.sig_bytes == 4 && p->hasher == KMU_HASHER_NOHASH) ? 20 : 52; // NoHashHasher of a u32 is < 2^32
    a.bk_mask = p->hasher == KMU_HASHER_INT64HASH ? 0xFFu : 0xFFFFu;
    hipFuncAttributes fa;
    KMU_HIP(ctx, hipFuncGetAttributes(&fa, (const void *) kern));
    size_t lds_max = 160 * 1024 - fa.sharedSizeBytes; // static LDS (none today) comes out of the same 160 KiB
    if (hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_max) != hipSuccess) {
        (void) hipGetLastError();
        lds_max = 64 * 1024;
    }
    const sketch_kernel_t kern_redo = k_sketch_pmh3a<false, false>; // takes what the PLAIN instantiation hands back
    if (plain && lds_max > 64 * 1024 &&
        hipFuncSetAttribute((const void *) kern_redo, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds_max) != hipSuccess)
        return fail(ctx, KMU_E_HIP, "hipFuncSetAttribute failed for the general sketch kernel");
    // LDS budget: dense keys 8 cap | weights 4 cap | slot minima 16 m | buckets 4 (NB+1) | misc | staged words
    // (bottom-k re-uses the staged-word area for its per-bucket distinct counts: NBUCKETS + 1 words)
    a.tile_words = (aa && !bottomk) ? 4 : (lds_max > 64 * 1024 || bottomk ? 4096 + 2 : 1024 + 2);
    size_t fixed = (size_t) 16 * a.m + 4 * ((size_t) NBUCKETS + 1 + 8) + 4 * (M_WORDS + 16 + DEF_PARTS) +
                   4 * ((size_t) a.tile_words + 4) + 64;
    if (fixed + 12 * 256 > lds_max) return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %d too large for LDS", a.m);
    uint32_t cap = (uint32_t) ((lds_max - fixed) / 12);
    cap &= ~63u;
    if (cap > 65472) cap = 65472; // positions are stored in 16 bits
    a.cap = cap;
    a.part_target = cap - cap / 10;
    a.inv_part_target = 1.0 / (double) a.part_target;
    if (plain && a.part_target > (uint32_t) KREG * 1024u)
        return fail(ctx, KMU_E_HIP, "internal: a single pass (%u k-mers) must fit the register keys of the PLAIN kernel", a.part_target);
    const uint32_t tp = (a.tile_words - 2) * 16; // 4096 or 1024 words of 16 bases
    a.tile_shift = 0;
    while ((1u << a.tile_shift) < tp) a.tile_shift++;
    if ((1u << a.tile_shift) != tp) return fail(ctx, KMU_E_HIP, "internal: tile size %u is not a power of two", tp);
    g->lds = (size_t) 12 * cap + fixed;
    KMU_TRY(alloc_queue(ctx, a));
    g->slots = (uint64_t) cus * std::max<int>(1, (int) (lds_max / g->lds));
    g->grid = (int) std::max<uint64_t>(1, std::min<uint64_t>((uint64_t) a.n_seq, g->slots));
    KMU_TRY(dev_array(ctx, "pmh.scr_keys", (size_t) g->grid * cap, &a.scr_keys));
    KMU_TRY(dev_array(ctx, "pmh.scr_info", (size_t) g->grid * cap, &a.scr_info));
    KMU_TRY(dev_array(ctx, "pmh.scr_w", (size_t) g->grid * cap, &a.scr_w));
    KMU_TRY(dev_array(ctx, "pmh.def_keys", (size_t) g->grid * DEF_CAP, &a.def_keys));
    if (plain) KMU_TRY(dev_array(ctx, "pmh.redo", (size_t) a.n_seq + 16, &a.redo_list));
    return KMU_OK;
}

// the general kernel over the n reads of a.redo_list (their count in queue[56], read back by the caller)
static int launch_listed(kmu_ctx *ctx, SketchArgs a, sketch_kernel_t kern, const PmhShape &g, uint32_t n, const char *name) {
    KMU_HIP(ctx, hipMemsetAsync(a.queue, 0, 256, ctx->stream));
    a.read_list = a.redo_list;
    a.n_queue = n;
    return launch_main(ctx, a, kern, (int) std::min<uint64_t>((uint64_t) n, g.slots), g.lds, name);
}

// the count of long / redo reads the last launch listed (a host synchronisation)
static int read_count(kmu_ctx *ctx, const SketchArgs &a, uint32_t *n) {
    return read_back(ctx, {{n, a.queue + 56}});
}

// every read of the batch has at most 256 k-mers: one wave per read builds its list (k_multiset_short), and one wave per
// list keeps all keys of a read in its registers, round by round (k_pmh_points_short)
static int launch_short(kmu_ctx *ctx, const SketchArgs &a, int cus) {
    const size_t lds_s = 4 * SHORT_WAVE_BYTES;
    const int per_cu = 5; // (88 registers: five waves per SIMD)
    KMU_TRY(launch(ctx, "k_multiset_short", k_multiset_short,
                   dim3((unsigned) std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t) a.n_seq + 3) / 4, (uint64_t) cus * per_cu))), dim3(256),
                   lds_s, a));
    KMU_HIP(ctx, hipMemsetAsync(a.queue, 0, 256, ctx->stream)); // (the points kernel's cursor)
    const sketch_kernel_t kpts = a.sig_bytes == 4 ? k_pmh_points_short<true> : k_pmh_points_short<false>;
    const size_t lds2 = (size_t) 4 * (2 * (size_t) a.m + 2) * 8 + WINV_LUT * 8;
    if (lds2 > 64 * 1024)
        KMU_HIP(ctx, hipFuncSetAttribute((const void *) kpts, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    const int per_cu2 = (int) std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds2));
    const int grid2 = (int) std::max<uint64_t>(1, std::min<uint64_t>(((uint64_t) a.n_seq + 3) / 4, (uint64_t) cus * per_cu2));
    return launch(ctx, "k_pmh_points_short", kpts, dim3(grid2), dim3(256), lds2, a);
}

// Whole unpacked DNA reads on the two-kernel route: the reads that fit one workgroup's registers (<= 10 240 k-mers: 87 % of
// the reads, 64 % of the bases of the ONT workload) go through k_multiset_uq, which does not sort what occurs once; the
// longer ones (and the rare read with too many repeated keys) are handed to the second shape; what that leaves -- reads of more than
// 20 480 places, 9.8 % of the k-mers -- to k_multiset_long, which cuts a read into sub-lists by key hash and runs the same step on
// each; and what THAT leaves (a read too repetitive for its sub-lists; none on the ONT workload) to the general list-emitting kernel
// (`kern`, reading its reads from a list; repetitive reads in rounds), launched only if the count read back is not zero.
static int launch_uq(kmu_ctx *ctx, SketchArgs a, sketch_kernel_t kern, const PmhShape &g, const PmhPlan &plan) {
    {
        const auto ka = k_multiset_uq<512, UQ1_BM, UQ1_COLL, 4>;
        const size_t lds_a = UqShape<512, UQ1_BM, UQ1_COLL>::LDS;
        KMU_HIP(ctx, hipFuncSetAttribute((const void *) ka, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        KMU_TRY(launch(ctx, "k_multiset_uq", ka, dim3((unsigned) std::max<uint64_t>(1, std::min<uint64_t>(a.n_seq, (uint64_t) plan.cus * 2))),
                       dim3(512), lds_a, a));
    }
    uint32_t n_long = 0;
    KMU_TRY(read_count(ctx, a, &n_long));
    if (n_long) { // the second shape: reads of up to 20 480 k-mers, from the first one's list
        const auto kb = k_multiset_uq<1024, UQ2_BM, UQ2_COLL, 4>;
        const size_t lds_b = UqShape<1024, UQ2_BM, UQ2_COLL>::LDS;
        uint32_t *rl2;
        KMU_TRY(dev_array(ctx, "pmh.redo2", (size_t) a.n_seq + 16, &rl2));
        KMU_HIP(ctx, hipFuncSetAttribute((const void *) kb, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        KMU_HIP(ctx, hipMemsetAsync(a.queue, 0, 256, ctx->stream));
        SketchArgs b = a;
        b.read_list = a.redo_list;
        b.redo_list = rl2;
        b.n_queue = n_long;
        KMU_TRY(launch(ctx, "k_multiset_uq", kb, dim3((unsigned) std::max<uint64_t>(1, std::min<uint64_t>(n_long, (uint64_t) plan.cus))), dim3(1024),
                       lds_b, b));
        KMU_TRY(read_count(ctx, a, &n_long));
        if (n_long) {
            // what the second shape leaves (reads of more than 20 480 places, and the rare shorter one with too many repeated keys):
            // k_multiset_long, one workgroup per CU over the general kernel's scratch (its grid is within pmh_shape's: def_keys is sized
            // by that).  It writes its own leftovers to the first shape's list, which nobody reads any more.  The timer's name is the
            // general kernel's: the sketch unit's stages are summed by name.
            KMU_HIP(ctx, hipFuncSetAttribute((const void *) k_multiset_long, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            KMU_HIP(ctx, hipMemsetAsync(a.queue, 0, 256, ctx->stream));
            SketchArgs c = a;
            c.read_list = rl2;
            c.n_queue = n_long;
            const uint64_t grid_c = std::min<uint64_t>(std::min<uint64_t>(n_long, (uint64_t) plan.cus), (uint64_t) g.grid);
            KMU_TRY(launch(ctx, "k_sketch_pmh3a", k_multiset_long, dim3((unsigned) std::max<uint64_t>(1, grid_c)), dim3(1024), lds_b, c));
            KMU_TRY(read_count(ctx, a, &n_long));
        }
    }
    // ... and the general kernel for the reads that one hands back: a sub-list beyond the registers, or too repetitive (none on the ONT workload)
    if (n_long) KMU_TRY(launch_listed(ctx, a, kern, g, n_long, "k_sketch_pmh3a"));
    KMU_HIP(ctx, hipMemsetAsync(a.queue, 0, 256, ctx->stream)); // (the points kernel's cursor; nothing is left to redo)
    return launch_points(ctx, a, plan.cus, plan.pts_long);
}

// PLAIN, one kernel; the sequences whose k-mers overflowed a pass (repetitive ones) are redone in rounds by the general
// instantiation, after the first launch (whose row for such a sequence is empty)
static int launch_one_pass(kmu_ctx *ctx, const SketchArgs &a, sketch_kernel_t kern, const PmhShape &g) {
    KMU_TRY(launch_main(ctx, a, kern, g.grid, g.lds, "k_sketch_pmh3a"));
    uint32_t n_redo = 0;
    KMU_TRY(read_count(ctx, a, &n_redo));
    if (n_redo) KMU_TRY(launch_listed(ctx, a, k_sketch_pmh3a<false, false>, g, n_redo, "k_sketch_pmh3a_redo"));
    return KMU_OK;
}

static SketchArgs sketch_args(const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const PmhInputs &in) {
    SketchArgs a;
    memset(&a, 0, sizeof a);
    a.skip_longer = in.skip_longer;
    a.hashed = in.hashed;
    a.hashed_bytes = in.hashed_bytes;
    a.part_h = in.part_h;
    a.part_k = in.part_k;
    a.bases = ds.bases;
    a.offsets = ds.offsets;
    a.packed_offsets = ds.packed_offsets;
    a.block_rows = in.d_block_rows;
    a.n_seq = ds.n_seq;
    a.n_queue = ds.n_seq;
    a.packed = ds.packed;
    a.total_bytes = ds.total_bytes;
    a.cfg = KmerCfg{p->kmer_type, in.hashed_bytes ? 1 : p->kmer_size, p->fhash};
    a.m = p->sketch_size;
    a.hasher = p->hasher;
    a.rand08 = (p->flags & KMU_FLAG_RAND08) ? 1 : 0;
    a.sig_bytes = kmer_val_bytes(p->kmer_type);
    a.block_size = (uint32_t) p->block_size;
    const uint32_t m32 = (uint32_t) a.m;
    const uint64_t m64 = (uint64_t) a.m;
    a.idx_thresh = (0u - m32) % m32;
    a.idx_zone = 0xFFFFFFFFFFFFFFFFull - (0xFFFFFFFFFFFFFFFFull - m64 + 1ull) % m64;
    // ExpRestricted01::new(lambda), lambda = ln(m / (m-1)) -- same libm expressions as the crate / the oracle
    double lambda = a.m >= 2 ? std::log((double) a.m / (double) (a.m - 1)) : 1.0;
    a.e01.lambda = lambda;
    a.e01.c1 = (std::exp(lambda) - 1.0) / lambda;
    a.e01.c2 = std::log(2.0 / (1.0 + std::exp(-lambda))) / lambda;
    a.e01.c3 = (1.0 - std::exp(-lambda)) / lambda;
    a.sig_out = d_sig;
    a.err = d_err;
    return a;
}

namespace kmu {

int launch_pmh3a(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const PmhInputs &in) {
    SketchArgs a = sketch_args(p, ds, d_sig, d_err, in);
    PmhPlan plan;
    KMU_TRY(pmh_route(ctx, p, ds, in, &plan));
    if (plan.lists) KMU_TRY(alloc_lists(ctx, a, plan.list_bases));
    if (plan.route == PmhRoute::SMALLK) return launch_smallk(ctx, a, plan);
    const bool bottomk = p->algo == KMU_ALGO_BOTTOMK, aa = kmer_is_aa(p->kmer_type) || in.hashed_bytes != 0;
    const bool plain = plan.route == PmhRoute::SHORT || plan.route == PmhRoute::UQ || plan.route == PmhRoute::ONE_PASS;
    const sketch_kernel_t kern = plan.lists                    ? k_sketch_pmh3a<false, false, true>
                                 : plan.route == PmhRoute::ONE_PASS ? k_sketch_pmh3a<false, false, false, true>
                                 : bottomk                     ? (aa ? k_sketch_pmh3a<true, true> : k_sketch_pmh3a<false, true>)
                                 : aa                          ? k_sketch_pmh3a<true, false>
                                                               : k_sketch_pmh3a<false, false>;
    a.counts_out = in.d_counts;
    PmhShape g;
    KMU_TRY(pmh_shape(ctx, p, a, kern, plain, plan.cus, &g));
    if (plan.lists) a.queue2 = a.queue + 48;
    switch (plan.route) {
    case PmhRoute::SHORT: return launch_short(ctx, a, plan.cus);
    case PmhRoute::UQ: return launch_uq(ctx, a, kern, g, plan);
    case PmhRoute::LISTS:
        KMU_TRY(launch_main(ctx, a, kern, g.grid, g.lds, "k_sketch_pmh3a"));
        return launch_points(ctx, a, plan.cus, plan.pts_long);
    case PmhRoute::ONE_PASS: return launch_one_pass(ctx, a, kern, g);
    default: return launch_main(ctx, a, kern, g.grid, g.lds, bottomk ? "k_sketch_bottomk" : "k_sketch_pmh3a");
    }
}

int launch_pmh3a_leaves(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *items, const uint64_t *bounds, uint32_t n_leaves,
                        uint64_t *part_h, uint64_t *part_k, uint32_t *d_err) {
    PmhInputs in;
    in.hashed = items;
    in.hashed_bytes = 8;
    in.part_h = part_h;
    in.part_k = part_k;
    return launch_pmh3a(ctx, p, hashed_seqs(items, bounds, n_leaves), nullptr, d_err, in);
}

int sketch_pmh_per_seq(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_block_rows, void *d_sig,
                       uint32_t *d_err, const uint64_t *h_offsets) {
    const uint32_t n_seq = ds.n_seq;
    // Sequences far longer than one LDS pass (genomes, not reads) would take L / cap passes in the per-sequence
    // kernel.  They go through the same global route as a sketch over all sequences -- hashes, radix partition
    // into leaves, per-leaf slot minima, merge -- one sequence at a time, which is linear in L.
    uint32_t skip_longer = 0;
    uint64_t len_stats[2] = {0, 0}; // longest sequence, all bases (whole sequences only)
    std::vector<uint32_t> long_seqs;
    PmhInputs in;
    in.d_block_rows = d_block_rows;
    if (p->block_size == 0 && smallk_route(p, 0, false, d_block_rows != nullptr)) // any length fits the histogram
        return launch_pmh3a(ctx, p, ds, d_sig, d_err, in);
    if (p->block_size == 0) {
        std::vector<uint64_t> h_off;
        if (h_offsets) {
            for (uint32_t i = 0; i < n_seq; i++) len_stats[0] = std::max(len_stats[0], h_offsets[i + 1] - h_offsets[i]);
            len_stats[1] = h_offsets[n_seq] - h_offsets[0];
        } else {
            void *mx;
            KMU_TRY(dev_buf(ctx, "pmh.maxlen", 64, &mx));
            KMU_HIP(ctx, hipMemsetAsync(mx, 0, 8, ctx->stream));
            const uint32_t mgrid = (uint32_t) std::min<uint64_t>(((uint64_t) n_seq + 1023) / 1024, (uint64_t) ctx->num_cus);
            KMU_TRY(launch(ctx, nullptr, k_max_len, dim3(mgrid ? mgrid : 1), dim3(1024), 0, ds.offsets, n_seq, (uint64_t *) mx));
            KMU_TRY(read_back(ctx, {{len_stats, mx, 16}}));
        }
        const uint64_t max_len = len_stats[0];
        if (max_len > (uint64_t) LONG_SEQ_KMERS + (uint64_t) p->kmer_size) {
            if (!h_offsets) {
                h_off.resize((size_t) n_seq + 1);
                KMU_HIP(ctx, hipMemcpyAsync(h_off.data(), ds.offsets, ((size_t) n_seq + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
                KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
                h_offsets = h_off.data();
            }
            for (uint32_t i = 0; i < n_seq; i++) {
                const uint64_t L = h_offsets[i + 1] - h_offsets[i];
                if (L >= (uint64_t) p->kmer_size && L - p->kmer_size + 1 > LONG_SEQ_KMERS) long_seqs.push_back(i);
            }
            skip_longer = LONG_SEQ_KMERS;
        }
    }
    in.skip_longer = skip_longer;
    in.len_stats = len_stats;
    KMU_TRY(launch_pmh3a(ctx, p, ds, d_sig, d_err, in));
    for (uint32_t i : long_seqs) {
        DevSeqs one = ds;
        one.offsets = ds.offsets + i;
        one.packed_offsets = ds.packed_offsets ? ds.packed_offsets + i : nullptr;
        one.n_seq = 1;
        const uint64_t *hk;
        uint64_t n_items = 0;
        KMU_TRY(hash_all_kmers(ctx, one, KmerCfg{p->kmer_type, p->kmer_size, p->fhash}, d_err, nullptr, &hk, &n_items));
        KMU_TRY(sketch_all_hashed(ctx, p, hk, n_items,
                                  reinterpret_cast<uint8_t *>(d_sig) + (size_t) i * p->sketch_size * sig_elem_bytes(p->sig_type), d_err));
    }
    return KMU_OK;
}

} // namespace kmu

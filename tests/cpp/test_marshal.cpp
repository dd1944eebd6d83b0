/*
 * test_marshal.cpp -- what every wrapper of include/kmerutils.hpp hands to the C-ABI, on recording stand-ins.  Stand-alone: no
 * device, no libkmu.so.  This translation unit defines the kmu_* entry points the covered wrappers reach; each appends one line to
 * a trace -- its name, then every argument: integers and parameter structs by value, every pointer as
 *     null | in:<name> (the base of a named input of the case) | out:<name> (the base of a named member of what the wrapper
 *     returned, resolved after it returns) | spare (any other non-null address)
 * -- then stores a scripted answer through its out-parameters and returns KMU_OK.  An array of zero elements is never named.
 * After a wrapper returns, `= name n` gives the size of every named member of its result.  A refusal is a line with its message.
 * The program prints the trace; tests/cpp/marshal_calls.txt is that output recorded once from the header as it was before its
 * marshalling steps were written once, and tests/test_cpp_marshal.py compares the two.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "kmerutils.hpp"

using namespace kmerutils;

// An address must not come back within a case, or a temporary that a wrapper freed would pass for the result allocated where it
// lay.  AddressSanitizer keeps freed blocks in quarantine; without it, what a case frees is held until the case ends.
#ifndef __SANITIZE_ADDRESS__
namespace {
void **g_held = nullptr;
size_t g_n_held = 0, g_cap_held = 0;
void release_held() {
    for (size_t i = 0; i < g_n_held; i++) free(g_held[i]);
    g_n_held = 0;
}
}  // namespace
void *operator new(size_t n) {
    if (void *p = malloc(n ? n : 1)) return p;
    throw std::bad_alloc();
}
void operator delete(void *p) noexcept {
    if (!p) return;
    if (g_n_held == g_cap_held) {
        g_cap_held = g_cap_held ? 2 * g_cap_held : 1024;
        g_held = static_cast<void **>(realloc(g_held, g_cap_held * sizeof(void *)));
    }
    g_held[g_n_held++] = p;
}
void operator delete(void *p, size_t) noexcept { operator delete(p); }
#else
namespace {
void release_held() {}
}  // namespace
#endif

// ---- the trace -----------------------------------------------------------------------------------------------------------------

namespace {

struct Tok {
    std::string text;
    const void *p = nullptr;
    bool is_ptr = false;
};
using Line = std::vector<Tok>;
struct Region {
    const void *p;
    std::string name;
};

std::vector<Line> g_lines;
std::vector<Region> g_in, g_out;
std::vector<std::string> g_sizes;
size_t g_n_lines = 0, g_n_cases = 0;

struct Script {
    uint64_t count = 3;      // what a count call answers, and the totals of the single-call wrappers (capped by their capacity)
    uint32_t n_components = 2;
    uint64_t n_slots = 2;
    uint64_t cells = 64;     // kmu_kfilter_cells_for
    int fail = 0;            // the next call returns this status
} g;

struct ByVal {
    std::string text;
};
/// a parameter struct by value: its 32-bit words (none of them has padding)
template <class P> ByVal V(const P *p) {
    static_assert(sizeof(P) % 4 == 0, "parameter structs are made of 32-bit words");
    if (!p) return {"null"};
    uint32_t w[sizeof(P) / 4];
    memcpy(w, p, sizeof(P));
    std::string s = "{";
    for (size_t i = 0; i < sizeof(P) / 4; i++) s += (i ? "," : "") + std::to_string(w[i]);
    return {s + "}"};
}
/// an opaque handle (context, counter, index, filter)
ByVal H(const void *h) { return {h ? "handle" : "null"}; }

void add(Line &l, const ByVal &v) { l.push_back({v.text, nullptr, false}); }
template <class T> std::enable_if_t<std::is_integral_v<T> || std::is_enum_v<T>> add(Line &l, T v) { l.push_back({std::to_string(v), nullptr, false}); }
template <class T> void add(Line &l, T *p) { l.push_back({"", p, true}); }

template <class... A> void T(const char *name, A... args) {
    Line l{{name, nullptr, false}};
    (add(l, args), ...);
    g_lines.push_back(std::move(l));
}
int rc() {
    const int r = g.fail;
    g.fail = 0;
    return r;
}

template <class Vec> void in(const std::string &name, const Vec &v) {
    if (!v.empty()) g_in.push_back({v.data(), name});
}
template <class Vec> void out(const std::string &name, const Vec &v) {
    if (!v.empty()) g_out.push_back({v.data(), name});
    g_sizes.push_back("= " + name + " " + std::to_string(v.size()));
}
void in(const std::string &name, const detail::Batch &b) {
    in(name + ".bytes", b.bytes);
    in(name + ".offsets", b.offsets);
    in(name + ".packed_offsets", b.packed_offsets);
    if (b.dev_bytes) g_in.push_back({b.dev_bytes, name + ".dev_bytes"});
    if (b.dev_offsets) g_in.push_back({b.dev_offsets, name + ".dev_offsets"});
}

std::string resolve(const void *p) {
    if (!p) return "null";
    for (const Region &r : g_in)
        if (r.p == p) return "in:" + r.name;
    for (const Region &r : g_out)
        if (r.p == p) return "out:" + r.name;
    return "spare";
}
void flush() {
    for (const Line &l : g_lines) {
        std::string s = l[0].text + "(";
        for (size_t i = 1; i < l.size(); i++) s += (i > 1 ? ", " : "") + (l[i].is_ptr ? resolve(l[i].p) : l[i].text);
        puts((s + ")").c_str());
        g_n_lines++;
    }
    for (const std::string &s : g_sizes) puts(s.c_str()), g_n_lines++;
    g_lines.clear();
    g_sizes.clear();
    g_in.clear();
    g_out.clear();
    release_held();
}
/// one case: its name, the calls it made, the sizes of what it returned -- or the message of its refusal
template <class F> void run(const char *name, F body) {
    printf("# %s\n", name);
    g_n_cases++;
    g_n_lines++;
    g = Script{};
    try {
        body();
    } catch (const KmuError &e) {
        g_sizes.push_back(std::string("KmuError ") + std::to_string(e.status()) + ": " + e.what());
    } catch (const std::exception &e) {
        g_sizes.push_back(std::string("refused: ") + e.what());
    }
    flush();
}

int fixed_ctx, fixed_counter, fixed_index, fixed_filter;   // the addresses of these are the handles

}  // namespace

// ---- the stand-ins -------------------------------------------------------------------------------------------------------------

extern "C" {

int kmu_create(const kmu_device_cfg *, kmu_ctx **out) { *out = reinterpret_cast<kmu_ctx *>(&fixed_ctx); return KMU_OK; }
void kmu_destroy(kmu_ctx *) {}
const char *kmu_last_error(const kmu_ctx *) { return "scripted failure"; }
int kmu_dev_alloc(kmu_ctx *, uint64_t bytes, void **out) { T("kmu_dev_alloc", bytes); *out = calloc(bytes ? bytes : 1, 1); return rc(); }
int kmu_dev_free(kmu_ctx *, void *p) { free(p); return KMU_OK; }
int kmu_copy_to_device(kmu_ctx *, void *dst, const void *src, uint64_t bytes) { T("kmu_copy_to_device", dst, src, bytes); memcpy(dst, src, bytes); return rc(); }
int kmu_copy_to_host(kmu_ctx *, void *dst, const void *src, uint64_t bytes) { T("kmu_copy_to_host", dst, src, bytes); memcpy(dst, src, bytes); return rc(); }
int kmu_set_hll_params(kmu_ctx *, const kmu_hll_params *hp) { T("kmu_set_hll_params", V(hp)); return rc(); }

int kmu_kmer_hashes(kmu_ctx *, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets, const uint64_t *packed, uint32_t n, uint64_t *o) {
    T("kmu_kmer_hashes", V(p), bases, offsets, packed, n, o);
    return rc();
}
int kmu_sketch(kmu_ctx *, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets, const uint64_t *packed, uint32_t n, const uint64_t *rows,
               void *sig, uint32_t *counts) {
    T("kmu_sketch", V(p), bases, offsets, packed, n, rows, sig, counts);
    return rc();
}
int kmu_sketch_groups(kmu_ctx *, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets, const uint64_t *packed, uint32_t n,
                      const uint64_t *group_offsets, uint32_t n_groups, void *sig) {
    T("kmu_sketch_groups", V(p), bases, offsets, packed, n, group_offsets, n_groups, sig);
    return rc();
}
int kmu_sketch_hashed(kmu_ctx *, const kmu_sketch_params *p, const void *hashed, const uint64_t *offsets, uint32_t n, void *sig, uint32_t *counts) {
    T("kmu_sketch_hashed", V(p), hashed, offsets, n, sig, counts);
    return rc();
}
/// two rows per sequence
int kmu_block_layout(const uint64_t *offsets, uint32_t n, uint32_t block_size, uint64_t *rows) {
    T("kmu_block_layout", offsets, n, block_size, rows);
    for (uint32_t i = 0; i <= n; i++) rows[i] = 2 * i;
    return rc();
}
int kmu_anchor_layout(const uint64_t *offsets, uint32_t n, uint32_t window, uint32_t overlap, uint64_t *rows) {
    T("kmu_anchor_layout", offsets, n, window, overlap, rows);
    for (uint32_t i = 0; i <= n; i++) rows[i] = 2 * i;
    return rc();
}
int kmu_read_anchors(kmu_ctx *, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n, uint32_t window, uint32_t overlap,
                     const uint64_t *rows, uint64_t *h, uint32_t *c, uint32_t *nn) {
    T("kmu_read_anchors", V(p), bases, offsets, n, window, overlap, rows, h, c, nn);
    return rc();
}

int kmu_sig_equal_pairs(kmu_ctx *, const void *a, uint32_t na, const void *b, uint32_t nb, uint32_t m, int sig_type, const uint32_t *ia, const uint32_t *ib,
                        uint64_t n_pairs, int mem, uint32_t *o) {
    T("kmu_sig_equal_pairs", a, na, b, nb, m, sig_type, ia, ib, n_pairs, mem, o);
    *o = 1;
    return rc();
}
int kmu_sig_knn(kmu_ctx *, const void *q, uint32_t nq, const void *db, uint32_t ndb, uint32_t m, int sig_type, uint32_t k, const uint32_t *gq,
                const uint32_t *gdb, int mem, uint32_t *idx, uint16_t *eq) {
    T("kmu_sig_knn", q, nq, db, ndb, m, sig_type, k, gq, gdb, mem, idx, eq);
    return rc();
}
int kmu_minhash_distance_pairs(kmu_ctx *, const uint64_t *a, uint32_t na, const uint64_t *b, uint32_t nb, uint32_t m, const uint32_t *ia, const uint32_t *ib,
                               uint64_t n_pairs, int mem, uint32_t *o) {
    T("kmu_minhash_distance_pairs", a, na, b, nb, m, ia, ib, n_pairs, mem, o);
    o[0] = 1, o[1] = 2, o[2] = 2;
    return rc();
}
int kmu_anchor_match(kmu_ctx *, const uint64_t *q, uint32_t nq, const uint64_t *db, uint32_t ndb, uint32_t m, uint32_t n_keys, uint32_t min_common,
                     const uint32_t *gq, const uint32_t *gdb, int mem, uint32_t *pairs, uint32_t *dist, uint64_t cap, uint64_t *n) {
    T("kmu_anchor_match", q, nq, db, ndb, m, n_keys, min_common, gq, gdb, mem, pairs, dist, cap, n);
    *n = g.count;
    return rc();
}
int kmu_anchor_overlaps(kmu_ctx *, const uint32_t *pairs, const uint32_t *dist, uint64_t n_pairs, const uint64_t *rows_q, uint32_t nq, const uint64_t *rows_db,
                        uint32_t ndb, uint32_t strands, uint32_t band, uint32_t min_score, uint32_t flags, int mem, kmu_overlap *o, uint64_t cap, uint64_t *n) {
    T("kmu_anchor_overlaps", pairs, dist, n_pairs, rows_q, nq, rows_db, ndb, strands, band, min_score, flags, mem, o, cap, n);
    *n = g.count;
    return rc();
}
int kmu_anchor_index_create(kmu_ctx *, const uint64_t *h, uint32_t ndb, uint32_t m, uint32_t n_keys, const uint32_t *group, int mem, kmu_anchor_index **o) {
    T("kmu_anchor_index_create", h, ndb, m, n_keys, group, mem);
    *o = reinterpret_cast<kmu_anchor_index *>(&fixed_index);
    return rc();
}
void kmu_anchor_index_destroy(kmu_anchor_index *ix) { T("kmu_anchor_index_destroy", H(ix)); }
int kmu_anchor_index_info(const kmu_anchor_index *ix, kmu_anchor_index_info_t *o) { T("kmu_anchor_index_info", H(ix), o); return rc(); }
int kmu_anchor_index_occupancy(kmu_anchor_index *ix, uint64_t *hist, uint32_t n_bins, int mem) { T("kmu_anchor_index_occupancy", H(ix), hist, n_bins, mem); return rc(); }
int kmu_anchor_index_match(kmu_anchor_index *ix, const uint64_t *q, uint32_t nq, const uint32_t *gq, uint32_t min_common, uint32_t max_occ, int mem,
                           uint32_t *pairs, uint32_t *dist, uint64_t cap, uint64_t *n) {
    T("kmu_anchor_index_match", H(ix), q, nq, gq, min_common, max_occ, mem, pairs, dist, cap, n);
    *n = g.count;
    return rc();
}
int kmu_components(kmu_ctx *, uint32_t n_nodes, const uint32_t *edges, uint64_t n_edges, uint32_t stride, uint32_t weight_at, uint32_t min_weight, int mem,
                   uint32_t *l, uint32_t *c, uint32_t *s, uint32_t *m, uint32_t *n) {
    T("kmu_components", n_nodes, edges, n_edges, stride, weight_at, min_weight, mem, l, c, s, m, n);
    *n = std::min(g.n_components, n_nodes);
    return rc();
}
int kmu_components_knn(kmu_ctx *, uint32_t n_nodes, const uint32_t *idx, const uint16_t *eq, uint32_t k, uint32_t min_eq, int mem, uint32_t *l, uint32_t *c,
                       uint32_t *s, uint32_t *m, uint32_t *n) {
    T("kmu_components_knn", n_nodes, idx, eq, k, min_eq, mem, l, c, s, m, n);
    *n = std::min(g.n_components, n_nodes);
    return rc();
}
/// one window per k-mer start
int kmu_minimizer_layout(const uint64_t *offsets, uint32_t n, uint32_t k, uint32_t w, uint64_t *win) {
    T("kmu_minimizer_layout", offsets, n, k, w, win);
    win[0] = 0;
    for (uint32_t i = 0; i < n; i++) win[i + 1] = win[i] + (offsets[i + 1] - offsets[i] >= k ? offsets[i + 1] - offsets[i] - k + 1 : 0);
    return rc();
}
int kmu_read_minimizers(kmu_ctx *, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n, uint32_t w, uint64_t *h, uint32_t *pos,
                        uint32_t *read, uint8_t *strand, uint64_t cap, uint64_t *mini_offsets, uint64_t *total) {
    T("kmu_read_minimizers", V(p), bases, offsets, n, w, h, pos, read, strand, cap, mini_offsets, total);
    *total = std::min(g.count, cap);
    return rc();
}
int kmu_seed_chains(kmu_ctx *, const uint32_t *pairs, uint64_t n_pairs, const uint32_t *pos_q, const uint32_t *read_q, const uint8_t *strand_q, uint32_t n_q,
                    uint32_t n_reads_q, const uint32_t *pos_db, const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                    const kmu_chain_params *p, int mem, kmu_chain *o, uint64_t cap, uint64_t *n) {
    T("kmu_seed_chains", pairs, n_pairs, pos_q, read_q, strand_q, n_q, n_reads_q, pos_db, read_db, strand_db, n_db, n_reads_db, V(p), mem, o, cap, n);
    *n = g.count;
    return rc();
}
int kmu_chain_align(kmu_ctx *, const kmu_chain *chains, uint64_t n_chains, const uint8_t *bq, const uint64_t *oq, uint32_t nq, const uint8_t *bdb,
                    const uint64_t *odb, uint32_t ndb, const kmu_align_params *p, int mem, kmu_chain_aln *o) {
    T("kmu_chain_align", chains, n_chains, bq, oq, nq, bdb, odb, ndb, V(p), mem, o);
    return rc();
}
int kmu_chain_cigar(kmu_ctx *, const kmu_chain *chains, uint64_t n_chains, const uint8_t *bq, const uint64_t *oq, uint32_t nq, const uint8_t *bdb,
                    const uint64_t *odb, uint32_t ndb, const kmu_cigar_params *p, int mem, kmu_chain_aln *aln, uint64_t *op_offsets, uint32_t *ops, uint64_t cap,
                    uint64_t *n) {
    T("kmu_chain_cigar", chains, n_chains, bq, oq, nq, bdb, odb, ndb, V(p), mem, aln, op_offsets, ops, cap, n);
    *n = g.count;
    return rc();
}
int kmu_chain_pileup(kmu_ctx *, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln, const uint64_t *op_offsets, const uint32_t *ops,
                     uint64_t n_ops, const uint8_t *bq, const uint64_t *oq, uint32_t nq, const uint8_t *bdb, const uint64_t *odb, uint32_t ndb,
                     const kmu_pileup_params *p, int mem, uint32_t *pile_q, uint32_t *pile_db) {
    T("kmu_chain_pileup", chains, n_chains, aln, op_offsets, ops, n_ops, bq, oq, nq, bdb, odb, ndb, V(p), mem, pile_q, pile_db);
    return rc();
}
int kmu_pile_call(kmu_ctx *, const uint32_t *pile, const uint8_t *bases, const uint64_t *offsets, uint32_t n, const kmu_pile_call_params *p, int mem,
                  uint8_t *call, kmu_read_pile *reads) {
    T("kmu_pile_call", pile, bases, offsets, n, V(p), mem, call, reads);
    return rc();
}
int kmu_pile_ins_plan(kmu_ctx *, const uint32_t *pile, const uint8_t *call, uint64_t n_bases, const kmu_ins_plan_params *p, int mem, uint8_t *ins_len,
                      uint64_t *n_slots) {
    T("kmu_pile_ins_plan", pile, call, n_bases, V(p), mem, ins_len, n_slots);
    *n_slots = g.n_slots;
    return rc();
}
int kmu_chain_pile_ins(kmu_ctx *, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln, const uint64_t *op_offsets, const uint32_t *ops,
                       uint64_t n_ops, const uint8_t *bq, const uint64_t *oq, uint32_t nq, const uint8_t *bdb, const uint64_t *odb, uint32_t ndb,
                       const kmu_pileup_params *p, int mem, const uint8_t *ins_len_q, uint64_t n_slots_q, uint32_t *ins_q, const uint8_t *ins_len_db,
                       uint64_t n_slots_db, uint32_t *ins_db) {
    T("kmu_chain_pile_ins", chains, n_chains, aln, op_offsets, ops, n_ops, bq, oq, nq, bdb, odb, ndb, V(p), mem, ins_len_q, n_slots_q, ins_q, ins_len_db,
      n_slots_db, ins_db);
    return rc();
}
int kmu_pile_consensus(kmu_ctx *, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots, const uint32_t *ins,
                       const uint8_t *bases, const uint64_t *offsets, uint32_t n, const kmu_consensus_params *p, int mem, uint64_t *cons_offsets, uint8_t *cons,
                       uint64_t cap, uint64_t *total) {
    T("kmu_pile_consensus", pile, call, ins_len, n_slots, ins, bases, offsets, n, V(p), mem, cons_offsets, cons, cap, total);
    *total = std::min(g.count, cap);
    return rc();
}
int kmu_pile_segments(kmu_ctx *, const uint32_t *pile, const uint64_t *offsets, uint32_t n, const kmu_pile_seg_params *p, int mem, uint64_t *seg_offsets,
                      kmu_pile_seg *segs, uint64_t cap, uint64_t *total, kmu_read_trim *reads) {
    T("kmu_pile_segments", pile, offsets, n, V(p), mem, seg_offsets, segs, cap, total, reads);
    *total = std::min(g.count, cap);
    return rc();
}
int kmu_extract_ranges(kmu_ctx *, const uint8_t *bases, uint64_t n_bases, const uint64_t *begin, const uint64_t *end, uint64_t n_ranges, int mem,
                       uint64_t *out_offsets, uint8_t *o, uint64_t cap, uint64_t *total) {
    T("kmu_extract_ranges", bases, n_bases, begin, end, n_ranges, mem, out_offsets, o, cap, total);
    *total = g.count;
    return rc();
}
int kmu_pile_consensus_pos(kmu_ctx *, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots, const uint32_t *ins,
                           const uint8_t *bases, const uint64_t *offsets, uint32_t n, const kmu_consensus_params *p, int mem, const uint64_t *rows,
                           uint64_t n_rows, uint64_t *pos) {
    T("kmu_pile_consensus_pos", pile, call, ins_len, n_slots, ins, bases, offsets, n, V(p), mem, rows, n_rows, pos);
    return rc();
}
int kmu_sg_classify(kmu_ctx *, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains, const uint64_t *offsets, uint32_t n,
                    const kmu_sg_params *p, int mem, uint8_t *classes, kmu_sg_read *reads) {
    T("kmu_sg_classify", chains, aln, n_chains, offsets, n, V(p), mem, classes, reads);
    return rc();
}
int kmu_sg_graph(kmu_ctx *, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains, const uint64_t *offsets, uint32_t n, const kmu_sg_params *p,
                 int mem, uint8_t *classes, kmu_sg_read *reads, kmu_sg_arc *arcs, uint64_t cap, uint64_t *arc_offsets, uint64_t *total) {
    T("kmu_sg_graph", chains, aln, n_chains, offsets, n, V(p), mem, classes, reads, arcs, cap, arc_offsets, total);
    *total = g.count;
    return rc();
}
int kmu_sg_unitigs(kmu_ctx *, const kmu_sg_arc *arcs, uint64_t n_arcs, const kmu_sg_read *reads, const uint64_t *offsets, uint32_t n, int mem,
                   kmu_sg_unitig *unitigs, kmu_sg_step *path, kmu_sg_place *place, uint64_t *n_steps, uint64_t *total) {
    T("kmu_sg_unitigs", arcs, n_arcs, reads, offsets, n, mem, unitigs, path, place, n_steps, total);
    *n_steps = std::min<uint64_t>(g.count, n);
    *total = std::min<uint64_t>(g.count / 2, n);
    return rc();
}
int kmu_sg_unitig_seqs(kmu_ctx *, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path, uint64_t n_steps, const uint8_t *bases,
                       const uint64_t *offsets, uint32_t n, int mem, uint64_t *seq_offsets, uint8_t *seq, uint64_t cap, uint64_t *total) {
    T("kmu_sg_unitig_seqs", unitigs, n_unitigs, path, n_steps, bases, offsets, n, mem, seq_offsets, seq, cap, total);
    *total = g.count;
    return rc();
}
int kmu_sg_clean(kmu_ctx *, const kmu_sg_arc *arcs, uint64_t n_arcs, const kmu_sg_read *reads, uint32_t n, const kmu_sg_clean_params *p, int mem,
                 kmu_sg_arc *arcs_out, kmu_sg_read *reads_out, kmu_sg_clean_stats *stats) {
    T("kmu_sg_clean", arcs, n_arcs, reads, n, V(p), mem, arcs_out, reads_out, stats);
    *stats = kmu_sg_clean_stats{1, g.count, 0, 0, 0, 1, 0, n_arcs};   // count 0: a round that removed nothing
    return rc();
}
int kmu_sg_unitig_chains(kmu_ctx *, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path, uint64_t n_steps, const kmu_sg_place *place,
                         const kmu_chain *chains, const uint8_t *classes, uint64_t n_chains, const uint64_t *offsets, uint32_t n, const kmu_um_params *p, int mem,
                         kmu_chain *o, kmu_um_stats *stats, uint64_t *total) {
    T("kmu_sg_unitig_chains", unitigs, n_unitigs, path, n_steps, place, chains, classes, n_chains, offsets, n, V(p), mem, o, stats, total);
    *total = std::min<uint64_t>(g.count, n);
    return rc();
}

int kmu_count_create(kmu_ctx *, const kmu_count_params *p, kmu_counter **o) {
    T("kmu_count_create", V(p));
    *o = reinterpret_cast<kmu_counter *>(&fixed_counter);
    return rc();
}
void kmu_count_destroy(kmu_counter *c) { T("kmu_count_destroy", H(c)); }
int kmu_count_add_reads(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, const uint64_t *packed, uint32_t n, int input_kind, int mem) {
    T("kmu_count_add_reads", H(c), bases, offsets, packed, n, input_kind, mem);
    return rc();
}
int kmu_count_add_kmers(kmu_counter *c, const uint64_t *kmers, uint64_t n, int mem) { T("kmu_count_add_kmers", H(c), kmers, n, mem); return rc(); }
int kmu_count_query(kmu_counter *c, const uint64_t *kmers, uint64_t n, int mem, uint32_t *o) { T("kmu_count_query", H(c), kmers, n, mem, o); return rc(); }
int kmu_count_nb_distinct(kmu_counter *c, uint64_t *o) { T("kmu_count_nb_distinct", H(c), o); *o = g.count; return rc(); }
int kmu_count_nb_unique(kmu_counter *c, uint64_t *o) { T("kmu_count_nb_unique", H(c), o); *o = g.count; return rc(); }
int kmu_count_dump(kmu_counter *c, uint32_t min_count, uint64_t *kmers, uint32_t *counts, uint64_t cap, uint64_t *n) {
    T("kmu_count_dump", H(c), min_count, kmers, counts, cap, n);
    *n = g.count;
    return rc();
}
int kmu_count_eliminate_once(kmu_counter *c) { T("kmu_count_eliminate_once", H(c)); return rc(); }
int kmu_count_once_positions(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n, int mem, uint64_t *kmers, uint32_t *numseq,
                             uint32_t *numkmer, uint64_t cap, uint64_t *total) {
    T("kmu_count_once_positions", H(c), bases, offsets, n, mem, kmers, numseq, numkmer, cap, total);
    *total = g.count;
    return rc();
}
int kmu_count_histogram(kmu_counter *c, uint64_t *hist, uint32_t n_bins, int mem) { T("kmu_count_histogram", H(c), hist, n_bins, mem); return rc(); }
int kmu_count_read_profile(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n, int mem, uint32_t solid_min, uint16_t *counts,
                           kmu_read_abundance *stats) {
    T("kmu_count_read_profile", H(c), bases, offsets, n, mem, solid_min, counts, stats);
    return rc();
}
int kmu_count_add_reads_filtered(kmu_counter *c, kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n, int mem, uint64_t *passed) {
    T("kmu_count_add_reads_filtered", H(c), H(f), bases, offsets, n, mem, passed);
    *passed = g.count;
    return rc();
}

uint64_t kmu_kfilter_cells_for(uint64_t expected, uint32_t bits) { T("kmu_kfilter_cells_for", expected, bits); return g.cells; }
int kmu_kfilter_create(kmu_ctx *, const kmu_kfilter_params *p, kmu_kfilter **o) {
    T("kmu_kfilter_create", V(p));
    *o = reinterpret_cast<kmu_kfilter *>(&fixed_filter);
    return rc();
}
void kmu_kfilter_destroy(kmu_kfilter *f) { T("kmu_kfilter_destroy", H(f)); }
int kmu_kfilter_add_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n, int mem) { T("kmu_kfilter_add_reads", H(f), bases, offsets, n, mem); return rc(); }
int kmu_kfilter_add_kmers(kmu_kfilter *f, const uint64_t *kmers, uint64_t n, int mem) { T("kmu_kfilter_add_kmers", H(f), kmers, n, mem); return rc(); }
int kmu_kfilter_query(kmu_kfilter *f, const uint64_t *kmers, uint64_t n, int mem, uint8_t *cls) { T("kmu_kfilter_query", H(f), kmers, n, mem, cls); return rc(); }
int kmu_kfilter_info(kmu_kfilter *f, kmu_kfilter_info_t *o) { T("kmu_kfilter_info", H(f), o); o->n_cells = 4; return rc(); }
int kmu_kfilter_export(kmu_kfilter *f, uint64_t *words, int mem) { T("kmu_kfilter_export", H(f), words, mem); return rc(); }
int kmu_kfilter_merge(kmu_kfilter *dst, const kmu_kfilter *src) { T("kmu_kfilter_merge", H(dst), H(src)); return rc(); }
int kmu_kfilter_select_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n, int mem, uint64_t *kmers, uint64_t cap, uint64_t *total) {
    T("kmu_kfilter_select_reads", H(f), bases, offsets, n, mem, kmers, cap, total);
    *total = g.count;
    return rc();
}
int kmu_ingest_fastx(kmu_ctx *, const uint8_t *text, uint64_t n_bytes, int mem, uint8_t *bases, uint64_t bases_cap, uint64_t *offsets, uint64_t offsets_cap,
                     uint32_t *record_index, kmu_ingest_info *info) {
    T("kmu_ingest_fastx", text, n_bytes, mem, bases, bases_cap, offsets, offsets_cap, record_index, info);
    *info = kmu_ingest_info{g.count, g.count, 10 * g.count, 10 * g.count, 0, 0};
    if (offsets)
        for (uint64_t i = 0; i < offsets_cap; i++) offsets[i] = 10 * i;
    return rc();
}

}  // extern "C"

// ---- inputs --------------------------------------------------------------------------------------------------------------------

namespace {

detail::Batch ascii(const std::vector<std::string> &reads) {
    detail::Batch b;
    b.offsets.assign(1, 0);
    for (const std::string &r : reads) {
        b.bytes.insert(b.bytes.end(), r.begin(), r.end());
        b.offsets.push_back(b.bytes.size());
    }
    if (!b.bytes.empty()) b.bytes.resize(b.bytes.size() + 16, 0);   // reads without bases: no byte at all
    return b;
}
/// a batch whose reads are "on the device": the pointers of a host batch that outlives it
detail::Batch resident(const detail::Batch &host) {
    detail::Batch b;
    b.offsets = host.offsets;
    b.dev_bytes = host.bytes.data();
    b.dev_offsets = host.offsets.data();
    return b;
}
const std::vector<std::string> TWO = {"ACGTACGTAC", "GGCATTGCAGTA"}, TWO_DB = {"TTGACCAGT", "CAGTACGTACG"};
const std::vector<std::string> NO_BASES = {"", ""};

std::vector<kmu_chain> chains_of(size_t n) {
    std::vector<kmu_chain> c(n, kmu_chain{});
    for (size_t i = 0; i < n; i++) c[i] = kmu_chain{0, 1, 0, 5, 3, 3, 0, 8, 1, 9};
    return c;
}
ChainCigars cigars_of(size_t n_chains, size_t n_ops) {
    ChainCigars c;
    c.aln.assign(n_chains, kmu_chain_aln{});
    c.op_offsets.assign(n_chains + 1, 0);
    c.ops.assign(n_ops, (8u << 4) | KMU_CIGAR_EQ);
    if (n_chains) c.op_offsets.back() = n_ops;
    return c;
}
void in(const std::string &name, const ChainCigars &c) {
    in(name + ".aln", c.aln);
    in(name + ".op_offsets", c.op_offsets);
    in(name + ".ops", c.ops);
}
void in(const std::string &name, const Minimizers &m) {
    in(name + ".hashes", m.hashes);
    in(name + ".pos", m.pos);
    in(name + ".read", m.read);
    in(name + ".strand", m.strand);
    in(name + ".offsets", m.offsets);
}
void in(const std::string &name, const Unitigs &u) {
    in(name + ".unitigs", u.unitigs);
    in(name + ".path", u.path);
    in(name + ".place", u.place);
}
Minimizers minimizers_of(uint32_t n_reads, uint32_t per_read, bool strand = true) {
    Minimizers m;
    m.offsets.assign(1, 0);
    for (uint32_t r = 0; r < n_reads; r++) {
        for (uint32_t e = 0; e < per_read; e++) {
            m.hashes.push_back(100 + e);
            m.pos.push_back(e);
            m.read.push_back(r);
            if (strand) m.strand.push_back(0);
        }
        m.offsets.push_back(m.hashes.size());
    }
    return m;
}
/// two reads on one unitig
Unitigs layout_of(uint32_t n_reads) {
    Unitigs u;
    if (n_reads) u.unitigs.push_back(kmu_sg_unitig{0, 12, n_reads, 0, 0, 0});
    for (uint32_t r = 0; r < n_reads; r++) {
        u.path.push_back(kmu_sg_step{r, 0, 10 + r});
        u.place.push_back(kmu_sg_place{0, r, 0, 0});
    }
    return u;
}
std::vector<ReadAnchors<Kmer32bit>> anchors_of(uint32_t n_reads) {
    std::vector<ReadAnchors<Kmer32bit>> reads(n_reads);
    for (uint32_t r = 0; r < n_reads; r++) {
        reads[r].readnum = 10 + r;
        for (uint32_t s = 0; s < 2; s++) reads[r].anchors.push_back(SliceAnchor<Kmer32bit>{10 + r, 4 * s, {{7 + s, 1}, {9, 2}}});
    }
    return reads;
}
void out(const std::string &name, const Components &c) {
    out(name + ".label", c.label);
    out(name + ".cluster", c.cluster);
    out(name + ".size", c.size);
    out(name + ".members", c.members);
}
void out(const std::string &name, const ConsensusReads &c) {
    out(name + ".bases", c.bases);
    out(name + ".offsets", c.offsets);
}
void out(const std::string &name, const ChainCigars &c) {
    out(name + ".aln", c.aln);
    out(name + ".ops", c.ops);
    out(name + ".op_offsets", c.op_offsets);
}
template <class Tables> void out_tables(const std::string &name, const Tables &t) {
    out(name + ".q", t.q);
    out(name + ".db", t.db);
    g_sizes.push_back("= " + name + ".shared " + std::to_string(int(t.shared)));
}
void out(const std::string &name, const Minimizers &m) {
    out(name + ".hashes", m.hashes);
    out(name + ".pos", m.pos);
    out(name + ".read", m.read);
    out(name + ".strand", m.strand);
    out(name + ".offsets", m.offsets);
}
void out(const std::string &name, const Unitigs &u) {
    out(name + ".unitigs", u.unitigs);
    out(name + ".path", u.path);
    out(name + ".place", u.place);
}
/// the result of a composite wrapper: its sizes only -- its calls went through temporaries whose addresses may be reused
template <class Vec> void size_of(const std::string &name, const Vec &v) { g_sizes.push_back("= " + name + " " + std::to_string(v.size())); }

// ---- the cases -----------------------------------------------------------------------------------------------------------------

void sketch_cases(Context &ctx) {
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    const std::vector<const Sequence *> ps = detail::pointers(seqs);
    const SeqSketcherParams params(3, 4, SketchAlgo::PROB3A, DataType::DNA);
    run("run_sketch_flat FHash, host batch", [&] {
        const detail::Batch b = detail::gather(ps);
        in("b", b);
        std::vector<uint32_t> flat;
        const size_t rows = detail::run_sketch_flat<Kmer32bit, uint32_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, kmer_revcomp_hash_fn, KMU_MODE_PER_SEQ, flat, 1);
        out("flat", flat);
        T("rows", rows);
    });
    run("run_sketch_flat FHash, all sequences, no read", [&] {
        const detail::Batch b = detail::gather(std::vector<const Sequence *>{});
        in("b", b);
        std::vector<uint32_t> flat;
        const size_t rows = detail::run_sketch_flat<Kmer32bit, uint32_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, kmer_revcomp_hash_fn, KMU_MODE_PER_SEQ, flat);
        out("flat", flat);
        T("rows", rows);
    });
    run("run_sketch_flat host callable", [&] {
        const detail::Batch b = detail::gather(ps);
        in("b", b);
        std::vector<uint32_t> flat;
        detail::run_sketch_flat<Kmer32bit, uint32_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, [](const Kmer32bit &k) { return k.get_compressed_value(); },
                                                     KMU_MODE_ALL_SEQS, flat);
        out("flat", flat);
    });
    run("run_sketch_flat host callable, no k-mer", [&] {
        const detail::Batch b = detail::gather(std::vector<const Sequence *>{});
        in("b", b);
        std::vector<uint32_t> flat;
        detail::run_sketch_flat<Kmer32bit, uint32_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, [](const Kmer32bit &k) { return k.get_compressed_value(); },
                                                     KMU_MODE_PER_SEQ, flat);
        out("flat", flat);
    });
    run("run_sketch_flat host callable, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO), b = resident(host);
        std::vector<uint32_t> flat;
        detail::run_sketch_flat<Kmer32bit, uint32_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, [](const Kmer32bit &k) { return k.get_compressed_value(); },
                                                     KMU_MODE_PER_SEQ, flat);
    });
    run("run_sketch_flat FHash, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO), b = resident(host);
        in("b", b);
        std::vector<uint64_t> flat;
        detail::run_sketch_flat<Kmer64bit, uint64_t>(ctx, b, KMU_ALGO_PROB3A, 3, 4, KMU_HASHER_NOHASH, kmer_revcomp_hash_fn, KMU_MODE_PER_SEQ, flat);
        out("flat", flat);
    });
    run("run_sketch_groups", [&] {
        const auto sigs = ProbHash3aSketch<Kmer32bit>(params, ctx).sketch_compressedkmer_seqs_groups({{ps[0]}, {ps[0], ps[1]}}, kmer_identity);
        size_of("sigs", sigs);
    });
    run("run_sketch_groups, no group", [&] {
        const auto sigs = ProbHash3aSketch<Kmer32bit>(params, ctx).sketch_compressedkmer_seqs_groups({}, kmer_identity);
        size_of("sigs", sigs);
    });
    run("HyperLogLogSketch", [&] {
        SetSketchParams hll;
        hll.m = 8;
        const HyperLogLogSketch<Kmer32bit, uint16_t> sk(params, hll, {}, ctx);
        size_of("per_seq", sk.sketch_compressedkmer(ps, kmer_identity));
        size_of("all_seqs", sk.sketch_compressedkmer_seqs(ps, kmer_identity));
        size_of("groups", sk.sketch_compressedkmer_seqs_groups({{ps[0]}, {ps[1]}}, kmer_identity));
    });
}

void signature_cases(Context &ctx) {
    const std::vector<uint32_t> a = {1, 2, 3, 4}, b = {1, 5, 3, 6};
    run("compute_probminhash_jaccard", [&] {
        in("a", a), in("b", b);
        T("jaccard_x100", int(100 * compute_probminhash_jaccard(a, b, ctx)));
    });
    run("compute_probminhash_jaccard, empty signatures", [&] { detail::equal_slots(ctx, std::vector<uint64_t>{}, std::vector<uint64_t>{}); });
    run("compute_probminhash_jaccard, different lengths", [&] { compute_probminhash_jaccard(a, std::vector<uint32_t>{1}, ctx); });
    run("compute_probminhash_jaccard, the library fails", [&] {
        g.fail = KMU_E_BAD_ARG;
        compute_probminhash_jaccard(a, b, ctx);
    });
    run("compute_superminhash_jaccard", [&] {
        const std::vector<double> x = {0.5, 1.5}, y = {0.5, 2.5};
        in("x", x), in("y", y);
        compute_superminhash_jaccard(x, y, ctx);
    });
    run("probminhash_get_jaccard_objects", [&] {
        in("a", a), in("b", b);
        size_of("common", *probminhash_get_jaccard_objects(a, b, ctx).second);
    });
    run("DistBlockSketched::eval", [&] {
        const BlockSketched x{0, 0, a}, y{1, 0, b};
        in("x", x.sketch), in("y", y.sketch);
        DistBlockSketched(ctx).eval(x, y);
        DistBlockSketched(ctx).eval(x, x);
    });
    const std::vector<uint32_t> q = {1, 2, 3, 4}, db = {1, 2, 5, 6, 7, 8}, gq = {0, 1}, gdb = {0, 1, 2};
    auto knn = [&](size_t nq, size_t ndb, bool groups) {
        in("q", q), in("db", db), in("gq", gq), in("gdb", gdb);
        std::vector<uint32_t> idx;
        std::vector<uint16_t> eq;
        sig_knn(q.data(), nq, db.data(), ndb, 2, 2, groups ? gq.data() : nullptr, groups ? gdb.data() : nullptr, idx, eq, ctx);
        out("idx", idx), out("eq", eq);
    };
    run("sig_knn", [&] { knn(2, 3, false); });
    run("sig_knn with groups", [&] { knn(2, 3, true); });
    run("sig_knn, no query row", [&] { knn(0, 3, false); });
    run("sig_knn, no database row", [&] { knn(2, 0, false); });
    const std::vector<std::vector<uint32_t>> rq = {{1, 2}, {3, 4}}, rdb = {{1, 2}, {5, 6}, {7, 8}};
    run("nearest_neighbours", [&] { size_of("lists", nearest_neighbours(rq, rdb, 2, nullptr, nullptr, ctx)); });
    run("nearest_neighbours with groups", [&] {
        in("gq", gq), in("gdb", gdb);
        size_of("lists", nearest_neighbours(rq, rdb, 2, &gq, &gdb, ctx));
    });
    run("nearest_neighbours, no query row", [&] { size_of("lists", nearest_neighbours({}, rdb, 2, nullptr, nullptr, ctx)); });
    run("nearest_neighbours, no row at all", [&] { size_of("lists", nearest_neighbours(std::vector<std::vector<uint32_t>>{}, {}, 2, nullptr, nullptr, ctx)); });
    run("nearest_neighbours, different lengths", [&] { nearest_neighbours(rq, {{1}}, 2, nullptr, nullptr, ctx); });
    run("jaccard_index_probminhash3a", [&] {
        const Sequence s("ACGTACGTAC");
        size_of("jac", jaccard_index_probminhash3a<Kmer32bit>(s, {Sequence("GGCATTGCAGTA"), Sequence("ACGTACGTAA")}, 4, 3, kmer_revcomp_hash_fn, ctx));
    });
}

void block_and_bottomk_cases(Context &ctx) {
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    const BlockSeqSketcher bs(5, 3, 4, ctx);
    run("blocksketch_sequences, host batch", [&] {
        const detail::Batch b = detail::gather(detail::pointers(seqs));
        in("b", b);
        size_of("seqs", bs.blocksketch_sequences(7, b, kmer_identity));
    });
    run("blocksketch_sequences, no read", [&] { size_of("seqs", bs.blocksketch_sequences(7, std::vector<const Sequence *>{}, kmer_identity)); });
    run("blocksketch_sequences, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO), b = resident(host);
        in("b", b);
        size_of("seqs", bs.blocksketch_sequences(7, b, kmer_identity));
    });
    run("blocksketch_sequence", [&] { size_of("blocks", bs.blocksketch_sequence(3, seqs[0], kmer_identity).sketch); });
    run("MinInvHashCountKmer::get_sketchcount", [&] {
        MinInvHashCountKmer<Kmer32bit> mh(4, ctx);
        size_of("empty", mh.get_sketchcount());
        mh.sketch_kmer_slice({Kmer32bit::build(5, 3), Kmer32bit::build(9, 3)});
        size_of("sketch", mh.get_sketchcount());
    });
    run("mininvhash_distance", [&] {
        MinInvHashCountKmer<Kmer32bit> x(4, ctx), y(4, ctx);
        x.sketch_kmer_slice({Kmer32bit::build(5, 3)});
        T("common", mininvhash_distance(x, y, ctx).common);
    });
    run("mininvhash_distance, different sizes", [&] { mininvhash_distance(MinInvHashCountKmer<Kmer32bit>(4, ctx), MinInvHashCountKmer<Kmer32bit>(5, ctx), ctx); });
    const Sequence s12("ACGTACGTACGTACGTACGT");
    run("sketch_seqrange_superminhash", [&] { size_of("sig", sketch_seqrange_superminhash(s12, {2, 18}, 9, 4, ctx)); });
    run("sketch_seqrange_superminhash, 16-mers", [&] { size_of("sig", sketch_seqrange_superminhash(s12, {0, 20}, 16, 4, ctx)); });
    run("sketch_seqrange_superminhash, bad range", [&] { sketch_seqrange_superminhash(s12, {5, 5}, 9, 4, ctx); });
    run("sketch_seqrange_superminhash, bad k", [&] { sketch_seqrange_superminhash(s12, {2, 18}, 8, 4, ctx); });
    run("sketch_seqrange_minhash", [&] { size_of("sketch", sketch_seqrange_minhash(s12, {2, 18}, 9, 4, ctx)); });
    run("sketch_seqrange_minhash, range past the end", [&] { sketch_seqrange_minhash(s12, {2, 21}, 9, 4, ctx); });
    run("minhash_distance", [&] { T("total", minhash_distance({{1, 1}, {4, 2}}, {{1, 1}}, ctx).total); });
    run("minhash_distance, empty sketches", [&] { T("total", minhash_distance({}, {}, ctx).total); });
}

void anchor_cases(Context &ctx) {
    const AnchorsGeneratorParameters params("reads.fa", 8, 2, 3, 4);
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    run("gen_read_anchors, packed sequences", [&] { size_of("reads", gen_read_anchors<Kmer32bit>(params, 10, detail::pointers(seqs), FHash::value_masked, KMU_HASHER_INT64HASH, ctx)); });
    run("gen_read_anchors, host batch", [&] {
        const detail::Batch b = ascii(TWO);
        in("b", b);
        size_of("reads", gen_read_anchors<Kmer32bit>(params, 10, b, FHash::canon_value, KMU_HASHER_INT64HASH, ctx));
    });
    run("gen_read_anchors, no read", [&] { size_of("reads", gen_read_anchors<Kmer32bit>(params, 10, ascii({}), FHash::value_masked, KMU_HASHER_INT64HASH, ctx)); });
    run("gen_read_anchors, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO), b = resident(host);
        in("b", b);
        size_of("reads", gen_read_anchors<Kmer32bit>(params, 10, b, FHash::value_masked, KMU_HASHER_INT64HASH, ctx));
    });

    const std::vector<uint64_t> h = {1, 2, 3, 4, 5, 6};   // 3 rows of 2
    const std::vector<uint32_t> grp = {0, 0, 1};
    auto index_match = [&](uint32_t nq, bool groups, uint64_t count) {
        in("h", h), in("grp", grp);
        const AnchorIndex ix(h, 3, 2, 1, groups ? grp : std::vector<uint32_t>{}, ctx);
        std::vector<uint32_t> pairs, dist;
        g.count = count;
        const uint64_t n = ix.match(h, nq, groups ? grp : std::vector<uint32_t>{}, 1, 5, pairs, dist);
        T("pairs", n);
        out("pairs", pairs), out("dist", dist);
    };
    run("AnchorIndex: create, info, occupancy", [&] {
        in("h", h);
        const AnchorIndex ix(h, 3, 2, 2, {}, ctx);
        ix.info();
        const std::vector<uint64_t> hist = ix.occupancy(4);
        out("hist", hist);
    });
    run("AnchorIndex with groups", [&] {
        in("h", h), in("grp", grp);
        const AnchorIndex ix(h, 3, 2, 1, grp, ctx);
    });
    run("AnchorIndex, no row", [&] { const AnchorIndex ix({}, 0, 2, 1, {}, ctx); });
    run("AnchorIndex, too few hashes", [&] { const AnchorIndex ix(h, 4, 2, 1, {}, ctx); });
    run("AnchorIndex, too few groups", [&] { const AnchorIndex ix(h, 3, 2, 1, {0}, ctx); });
    run("AnchorIndex::match, 3 pairs", [&] { index_match(3, false, 3); });
    run("AnchorIndex::match, 0 pairs", [&] { index_match(3, false, 0); });
    run("AnchorIndex::match with groups", [&] { index_match(3, true, 3); });
    run("AnchorIndex::match, no query row", [&] { index_match(0, false, 0); });
    run("AnchorIndex::match, too few hashes", [&] { index_match(4, false, 0); });

    auto matches = [&](uint32_t n_reads, uint32_t max_occ, uint64_t count) {
        const auto reads = anchors_of(n_reads);
        g.count = count;
        size_of("matches", match_read_anchors(reads, params, 1, 1, max_occ, ctx));
    };
    run("match_read_anchors, 3 pairs", [&] { matches(2, 0, 3); });
    run("match_read_anchors, 0 pairs", [&] { matches(2, 0, 0); });
    run("match_read_anchors with a repeat mask", [&] { matches(2, 5, 3); });
    run("match_read_anchors, no read", [&] { matches(0, 0, 0); });
    run("match_read_anchors with a repeat mask, no read", [&] { matches(0, 5, 0); });

    const std::vector<uint32_t> pairs = {0, 1, 1, 2}, dist = {1, 2, 0, 2, 2, 1};
    const std::vector<uint64_t> rows_q = {0, 2, 4}, rows_db = {0, 1, 3};
    auto overlaps = [&](bool with_pairs, bool with_dist, uint64_t count, bool upper = false) {
        in("pairs", pairs), in("dist", dist), in("rows_q", rows_q), in("rows_db", rows_db);
        g.count = count;
        const auto o = anchor_overlaps(with_pairs ? pairs : std::vector<uint32_t>{}, with_dist ? dist : std::vector<uint32_t>{}, rows_q, rows_db, 2, 1, 1, upper, ctx);
        out("records", o);
    };
    run("anchor_overlaps, 3 records", [&] { overlaps(true, true, 3); });
    run("anchor_overlaps, 0 records", [&] { overlaps(true, true, 0); });
    run("anchor_overlaps, upper, no dist", [&] { overlaps(true, false, 3, true); });
    run("anchor_overlaps, no pair", [&] { overlaps(false, false, 0); });
    run("anchor_overlaps, dist of another length", [&] { overlaps(false, true, 0); });
    run("anchor_overlaps, no row offsets", [&] { anchor_overlaps(pairs, dist, {}, rows_db, 2, 1, 1, false, ctx); });
    run("read_overlaps", [&] { size_of("overlaps", read_overlaps(anchors_of(2), params, 1, 1, 2, 1, 2, 0, ctx)); });
    run("read_overlaps, no read", [&] {
        g.count = 0;
        size_of("overlaps", read_overlaps(anchors_of(0), params, 1, 1, 2, 1, 2, 0, ctx));
    });
    run("read_clusters", [&] {
        const ReadClusters c = read_clusters(anchors_of(2), params, 1, 1, 2, 1, 2, 0, false, ctx);
        size_of("cluster", c.cluster), size_of("size", c.size), size_of("members", c.members);
    });
    run("read_clusters by votes, repeat mask", [&] {
        const ReadClusters c = read_clusters(anchors_of(2), params, 1, 1, 2, 1, 2, 4, true, ctx);
        size_of("cluster", c.cluster), size_of("size", c.size), size_of("members", c.members);
    });
}

void component_cases(Context &ctx) {
    const std::vector<uint32_t> edges = {0, 1, 9, 1, 2, 4};
    run("components", [&] {
        in("edges", edges);
        out("c", components(edges, 3, 3, 2, 5, ctx));
    });
    run("components, no edge", [&] { out("c", components(std::vector<uint32_t>{}, 3, 2, 0, 0, ctx)); });
    run("components, no node", [&] { out("c", components(std::vector<uint32_t>{}, 0, 2, 0, 0, ctx)); });
    run("components, one component among three nodes", [&] {
        in("edges", edges);
        g.n_components = 1;
        out("c", components(edges, 3, 3, 0, 0, ctx));
    });
    run("components, records of 3 words in a stride of 2", [&] { components(edges, 3, 4, 0, 0, ctx); });
    run("components, stride 1", [&] { components(edges, 3, 1, 0, 0, ctx); });
    const std::vector<kmu_overlap> records(2, kmu_overlap{0, 1, 0, 0, 3, 2, 0, 1});
    run("components of overlap records", [&] {
        in("records", records);
        out("c", components(records, 3, 2, false, ctx));
    });
    run("components of overlap records by votes, no record", [&] { out("c", components(std::vector<kmu_overlap>{}, 3, 2, true, ctx)); });
    const std::vector<uint32_t> idx = {1, 2, 0, 2, 0, 1};
    const std::vector<uint16_t> eq = {3, 1, 3, 0, 1, 0};
    run("components_knn", [&] {
        in("idx", idx), in("eq", eq);
        out("c", components_knn(idx, eq, 3, 2, 2, ctx));
    });
    run("components_knn, no eq", [&] {
        in("idx", idx);
        out("c", components_knn(idx, {}, 3, 2, 0, ctx));
    });
    run("components_knn, no node", [&] { out("c", components_knn({}, {}, 0, 2, 0, ctx)); });
    run("components_knn, idx of another size", [&] { components_knn(idx, eq, 2, 2, 0, ctx); });
    run("components_knn, eq of another size", [&] { components_knn(idx, {1}, 3, 2, 0, ctx); });
}

void minimizer_cases(Context &ctx) {
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    run("kmer_hashes", [&] {
        const detail::Batch b = ascii(TWO);
        in("b", b);
        out("hashes", kmer_hashes<Kmer32bit>(b, 5, FHash::canon_invhash, ctx));
    });
    run("kmer_hashes, packed sequences", [&] {
        const detail::Batch b = detail::gather(detail::pointers(seqs));
        in("b", b);
        out("hashes", kmer_hashes<Kmer64bit>(b, 5, FHash::canon_raw, ctx));
    });
    run("kmer_hashes, no read", [&] { out("hashes", kmer_hashes<Kmer32bit>(ascii({}), 5, FHash::canon_invhash, ctx)); });
    run("kmer_hashes, reads without bases", [&] { out("hashes", kmer_hashes<Kmer32bit>(ascii(NO_BASES), 5, FHash::canon_invhash, ctx)); });
    run("kmer_hashes, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO);
        kmer_hashes<Kmer32bit>(resident(host), 5, FHash::canon_invhash, ctx);
    });
    run("minimizer_layout", [&] {
        const detail::Batch b = ascii(TWO);
        in("b", b);
        out("win", minimizer_layout(b, 5, 3));
    });
    run("minimizer_layout, the library refuses", [&] {
        g.fail = KMU_E_BAD_ARG;
        minimizer_layout(ascii(TWO), 5, 0);
    });
    auto mini = [&](const detail::Batch &b, FHash f) {
        in("b", b);
        out("m", read_minimizers<Kmer32bit>(b, 5, 3, f, ctx));
    };
    run("read_minimizers", [&] { mini(ascii(TWO), FHash::canon_invhash); });
    run("read_minimizers, ntHash order: no strand", [&] { mini(ascii(TWO), FHash::canon_nthash); });
    run("read_minimizers, packed sequences", [&] { out("m", read_minimizers<Kmer32bit>(detail::pointers(seqs), 5, 3, FHash::canon_invhash, ctx)); });
    run("read_minimizers, no read", [&] { mini(ascii({}), FHash::canon_invhash); });
    run("read_minimizers, reads without bases", [&] { mini(ascii(NO_BASES), FHash::canon_invhash); });
    run("read_minimizers, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO);
        mini(resident(host), FHash::canon_invhash);
    });

    const std::vector<uint32_t> pairs = {0, 1, 1, 0};
    kmu_chain_params p{};
    p.span = 5, p.max_gap = 100, p.band = 10, p.min_seeds = 2, p.flags = KMU_CHAIN_UPPER;
    auto chains = [&](const Minimizers &q, const Minimizers &db, bool with_pairs, uint64_t count) {
        in("pairs", pairs), in("q", q), in("db", db);
        g.count = count;
        out("chains", seed_chains(with_pairs ? pairs : std::vector<uint32_t>{}, q, db, p, ctx));
    };
    run("seed_chains, 3 chains", [&] { chains(minimizers_of(2, 2), minimizers_of(2, 1), true, 3); });
    run("seed_chains, 0 chains", [&] { chains(minimizers_of(2, 2), minimizers_of(2, 1), true, 0); });
    run("seed_chains, self-join", [&] {
        const Minimizers q = minimizers_of(2, 2);
        in("pairs", pairs), in("q", q);
        out("chains", seed_chains(pairs, q, q, p, ctx));
    });
    run("seed_chains, no strands", [&] { chains(minimizers_of(2, 2, false), minimizers_of(2, 1, false), true, 3); });
    run("seed_chains, no pair", [&] { chains(minimizers_of(2, 2), minimizers_of(2, 1), false, 0); });
    run("seed_chains, reads without minimizers", [&] { chains(minimizers_of(2, 0), minimizers_of(2, 0), false, 0); });
    run("seed_chains, no offsets", [&] { chains(Minimizers{}, minimizers_of(2, 1), true, 0); });
    run("seed_chains, strands of another length", [&] {
        Minimizers q = minimizers_of(2, 2);
        q.strand.pop_back();
        chains(q, minimizers_of(2, 1), true, 0);
    });
    run("seed_pairs, self-join", [&] {
        const Minimizers q = minimizers_of(2, 2);
        in("q", q);
        size_of("pairs", seed_pairs(q, nullptr, 4, ctx));
    });
    run("seed_pairs, two sets", [&] {
        const Minimizers q = minimizers_of(2, 2), db = minimizers_of(2, 1);
        in("q", q), in("db", db);
        size_of("pairs", seed_pairs(q, &db, 0, ctx));
    });
    run("seed_pairs, no minimizer", [&] { size_of("pairs", seed_pairs(minimizers_of(2, 0), nullptr, 0, ctx)); });
    run("chain_hits, self-join", [&] {
        const Minimizers q = minimizers_of(2, 2);
        in("q", q);
        size_of("chains", chain_hits(q, nullptr, 5, 0, 5000, 500, 3, 0, ctx));
    });
    run("chain_hits, two sets", [&] {
        const Minimizers q = minimizers_of(2, 2), db = minimizers_of(2, 1);
        in("q", q), in("db", db);
        size_of("chains", chain_hits(q, &db, 5, 2, 100, 10, 2, 1, ctx));
    });
    run("read_chains", [&] {
        const detail::Batch b = ascii(TWO);
        in("b", b);
        size_of("chains", read_chains<Kmer32bit>(b, 5, 3, FHash::canon_invhash, 0, 5000, 500, 3, 0, ctx));
    });
}

/// the two-sided wrappers: the self-join and the two-batch form
template <class F> void two_sided(const char *what, F body) {
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    run((std::string(what) + ", self-join").c_str(), [&] {
        const detail::Batch q = ascii(TWO);
        in("q", q);
        body(q, nullptr);
    });
    run((std::string(what) + ", two batches").c_str(), [&] {
        const detail::Batch q = ascii(TWO), db = ascii(TWO_DB);
        in("q", q), in("db", db);
        body(q, &db);
    });
    run((std::string(what) + ", packed q and an ASCII db").c_str(), [&] {
        const detail::Batch q = detail::gather(detail::pointers(seqs)), db = ascii(TWO_DB);
        in("q", q), in("db", db);
        body(q, &db);
    });
    run((std::string(what) + ", device-resident q").c_str(), [&] {
        const detail::Batch host = ascii(TWO);
        body(resident(host), nullptr);
    });
    run((std::string(what) + ", device-resident db").c_str(), [&] {
        const detail::Batch host = ascii(TWO), db = resident(host);
        body(host, &db);
    });
}

void chain_cases(Context &ctx) {
    const std::vector<kmu_chain> chains = chains_of(2), no_chains;
    two_sided("chain_align", [&](const detail::Batch &q, const detail::Batch *db) {
        in("chains", chains);
        out("aln", chain_align(chains, q, db, 32, ctx));
    });
    run("chain_align, no chain", [&] { out("aln", chain_align(no_chains, ascii(TWO), nullptr, 64, ctx)); });
    run("align_chains", [&] {
        in("chains", chains);
        out("aln", align_chains(chains, ascii(TWO), nullptr, 64, ctx));
    });
    run("read_alignments", [&] {
        const auto r = read_alignments<Kmer32bit>(ascii(TWO), 5, 3, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, ctx);
        size_of("chains", r.first), size_of("aln", r.second);
    });

    for (uint64_t count : {3, 0})
        two_sided(count ? "chain_cigar, 3 runs" : "chain_cigar, 0 runs", [&](const detail::Batch &q, const detail::Batch *db) {
            in("chains", chains);
            g.count = count;
            out("cigars", chain_cigar(chains, q, db, 32, 1 << 20, ctx));
        });
    run("chain_cigar, no chain", [&] { out("cigars", chain_cigar(no_chains, ascii(TWO), nullptr, 64, 0, ctx)); });
    run("cigar_chains", [&] {
        in("chains", chains);
        out("cigars", cigar_chains(chains, ascii(TWO), nullptr, 64, 0, ctx));
    });

    const ChainCigars cigars = cigars_of(2, 3), no_cigars = cigars_of(0, 0), no_runs = cigars_of(2, 0);
    for (uint32_t sides : {KMU_PILE_Q | KMU_PILE_DB, KMU_PILE_Q, KMU_PILE_DB})
        two_sided(("chain_pileup, sides " + std::to_string(sides)).c_str(), [&](const detail::Batch &q, const detail::Batch *db) {
            in("chains", chains), in("cigars", cigars);
            out_tables("pile", chain_pileup(chains, cigars, q, db, sides, {}, ctx));
        });
    run("chain_pileup, no chain", [&] { out_tables("pile", chain_pileup(no_chains, no_cigars, ascii(TWO), nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx)); });
    run("chain_pileup, chains without runs", [&] {
        in("chains", chains), in("cigars", no_runs);
        out_tables("pile", chain_pileup(chains, no_runs, ascii(TWO), nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx));
    });
    for (uint32_t sides : {KMU_PILE_Q | KMU_PILE_DB, KMU_PILE_Q, KMU_PILE_DB})
        run(("chain_pileup, a db batch without bases, sides " + std::to_string(sides)).c_str(), [&] {
            const detail::Batch q = ascii(TWO), db = ascii(NO_BASES);
            in("chains", chains), in("cigars", cigars);
            out_tables("pile", chain_pileup(chains, cigars, q, &db, sides, {}, ctx));
        });
    run("chain_pileup, reads without bases", [&] {
        in("chains", chains), in("cigars", cigars);
        out_tables("pile", chain_pileup(chains, cigars, ascii(NO_BASES), nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx));
    });
    run("chain_pileup into the tables of an earlier call", [&] {
        const detail::Batch q = ascii(TWO), db = ascii(TWO_DB);
        ChainPileups into;
        into.q.assign(22 * KMU_PILE_COLS, 1);
        into.db.assign(20 * KMU_PILE_COLS, 1);
        in("chains", chains), in("cigars", cigars), in("into.q", into.q), in("into.db", into.db);
        out_tables("pile", chain_pileup(chains, cigars, q, &db, KMU_PILE_Q | KMU_PILE_DB, std::move(into), ctx));
    });
    run("chain_pileup, records of other chains", [&] { chain_pileup(chains, no_cigars, ascii(TWO), nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx); });
    run("pileup_chains", [&] {
        in("chains", chains), in("cigars", cigars);
        out_tables("pile", pileup_chains(chains, cigars, ascii(TWO), nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx));
    });
}

InsPlan plan_of(size_t n_bases, uint64_t n_slots) {
    InsPlan p;
    p.ins_len.assign(n_bases, 0);
    p.n_slots = n_slots;
    return p;
}

void correction_cases(Context &ctx) {
    const detail::Batch two = ascii(TWO), no_reads = ascii({}), no_bases = ascii(NO_BASES);
    const std::vector<uint32_t> table(22 * KMU_PILE_COLS, 2), no_table;
    const std::vector<uint8_t> call(22, 1), no_call;
    auto calls = [&](const std::vector<uint32_t> &t, const detail::Batch &b) {
        in("table", t), in("b", b);
        const PileCalls c = pile_call(t, b, 2, ctx);
        out("call", c.call), out("reads", c.reads);
    };
    run("pile_call", [&] { calls(table, two); });
    run("pile_call, packed sequences", [&] {
        const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
        calls(table, detail::gather(detail::pointers(seqs)));
    });
    run("pile_call, no read", [&] { calls(no_table, no_reads); });
    run("pile_call, reads without bases", [&] { calls(no_table, no_bases); });
    run("pile_call, a table of another batch", [&] { calls(no_table, two); });
    run("pile_call, device-resident batch", [&] { calls(table, resident(two)); });
    auto ins_plan = [&](const std::vector<uint32_t> &t, const std::vector<uint8_t> &c) {
        in("table", t), in("call", c);
        const InsPlan p = pile_ins_plan(t, c, 4, ctx);
        out("ins_len", p.ins_len);
        T("n_slots", p.n_slots);
    };
    run("pile_ins_plan", [&] { ins_plan(table, call); });
    run("pile_ins_plan, no base", [&] { ins_plan(no_table, no_call); });
    run("pile_ins_plan, calls of another batch", [&] { ins_plan(table, no_call); });

    const std::vector<kmu_chain> chains = chains_of(2), no_chains;
    const ChainCigars cigars = cigars_of(2, 3), no_cigars = cigars_of(0, 0);
    const InsPlan plan_q = plan_of(22, 2), plan_db = plan_of(20, 3), no_slots_q = plan_of(22, 0), no_slots_db = plan_of(20, 0);
    for (uint32_t sides : {KMU_PILE_Q | KMU_PILE_DB, KMU_PILE_Q, KMU_PILE_DB})
        two_sided(("chain_pile_ins, sides " + std::to_string(sides)).c_str(), [&](const detail::Batch &q, const detail::Batch *db) {
            in("chains", chains), in("cigars", cigars), in("plan_q", plan_q.ins_len), in("plan_db", plan_db.ins_len);
            out_tables("ins", chain_pile_ins(chains, cigars, q, plan_q, db, db ? &plan_db : nullptr, sides, {}, ctx));
        });
    for (uint32_t sides : {KMU_PILE_Q | KMU_PILE_DB, KMU_PILE_Q, KMU_PILE_DB}) {
        run(("chain_pile_ins, plans without slots, self-join, sides " + std::to_string(sides)).c_str(), [&] {
            in("chains", chains), in("cigars", cigars), in("plan_q", no_slots_q.ins_len);
            out_tables("ins", chain_pile_ins(chains, cigars, two, no_slots_q, nullptr, nullptr, sides, {}, ctx));
        });
        run(("chain_pile_ins, plans without slots, two batches, sides " + std::to_string(sides)).c_str(), [&] {
            const detail::Batch db = ascii(TWO_DB);
            in("chains", chains), in("cigars", cigars), in("plan_q", no_slots_q.ins_len), in("plan_db", no_slots_db.ins_len);
            out_tables("ins", chain_pile_ins(chains, cigars, two, no_slots_q, &db, &no_slots_db, sides, {}, ctx));
        });
    }
    run("chain_pile_ins, no chain", [&] { out_tables("ins", chain_pile_ins(no_chains, no_cigars, two, plan_q, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx)); });
    run("chain_pile_ins, reads without bases", [&] {
        const InsPlan none = plan_of(0, 0);
        in("chains", chains), in("cigars", cigars);
        out_tables("ins", chain_pile_ins(chains, cigars, no_bases, none, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx));
    });
    run("chain_pile_ins into the tables of an earlier call", [&] {
        ChainInsertions into;
        into.q.assign(2 * KMU_INS_COLS, 1);
        in("chains", chains), in("cigars", cigars), in("plan_q", plan_q.ins_len), in("into.q", into.q);
        out_tables("ins", chain_pile_ins(chains, cigars, two, plan_q, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, std::move(into), ctx));
    });
    run("chain_pile_ins, a db batch without its plan", [&] {
        const detail::Batch db = ascii(TWO_DB);
        chain_pile_ins(chains, cigars, two, plan_q, &db, nullptr, KMU_PILE_Q, {}, ctx);
    });
    run("chain_pile_ins, a plan of another batch", [&] { chain_pile_ins(chains, cigars, two, plan_db, nullptr, nullptr, KMU_PILE_Q, {}, ctx); });
    run("chain_pile_ins, records of other chains", [&] { chain_pile_ins(chains, no_cigars, two, plan_q, nullptr, nullptr, KMU_PILE_Q, {}, ctx); });
    run("insertions_chains", [&] {
        in("chains", chains), in("cigars", cigars), in("plan_q", plan_q.ins_len);
        out_tables("ins", insertions_chains(chains, cigars, two, plan_q, nullptr, nullptr, KMU_PILE_Q | KMU_PILE_DB, {}, ctx));
    });

    const std::vector<uint32_t> ins(2 * KMU_INS_COLS, 1), no_ins;
    auto consensus = [&](const std::vector<uint32_t> &t, const std::vector<uint8_t> &c, const InsPlan &p, const std::vector<uint32_t> &i, const detail::Batch &b,
                         bool alias = false) {
        in("table", t), in("call", c), in("plan", p.ins_len), in("ins", i), in("b", b);
        out("cons", alias ? consensus_reads(t, c, p, i, b, ctx) : pile_consensus(t, c, p, i, b, ctx));
    };
    run("pile_consensus", [&] { consensus(table, call, plan_q, ins, two); });
    run("pile_consensus, a long consensus", [&] {
        g.count = 100;
        consensus(table, call, plan_q, ins, two);
    });
    run("pile_consensus, no slot", [&] { consensus(table, call, no_slots_q, no_ins, two); });
    run("pile_consensus, no read", [&] { consensus(no_table, no_call, plan_of(0, 0), no_ins, no_reads); });
    run("pile_consensus, reads without bases", [&] { consensus(no_table, no_call, plan_of(0, 0), no_ins, no_bases); });
    run("pile_consensus, slots of another plan", [&] { consensus(table, call, plan_q, no_ins, two); });
    run("pile_consensus, device-resident batch", [&] { consensus(table, call, plan_q, ins, resident(two)); });
    run("consensus_reads", [&] { consensus(table, call, plan_q, ins, two, true); });

    const std::vector<uint64_t> rows = {0, 10, 22}, no_rows;
    auto positions = [&](const std::vector<uint32_t> &t, const std::vector<uint8_t> &c, const InsPlan &p, const std::vector<uint32_t> &i, const detail::Batch &b,
                         const std::vector<uint64_t> &r) {
        in("table", t), in("call", c), in("plan", p.ins_len), in("ins", i), in("b", b), in("rows", r);
        out("pos", pile_consensus_pos(t, c, p, i, b, r, ctx));
    };
    run("pile_consensus_pos", [&] { positions(table, call, plan_q, ins, two, rows); });
    run("pile_consensus_pos, no row", [&] { positions(table, call, plan_q, ins, two, no_rows); });
    run("pile_consensus_pos, no slot", [&] { positions(table, call, no_slots_q, no_ins, two, rows); });
    run("pile_consensus_pos, reads without bases", [&] { positions(no_table, no_call, plan_of(0, 0), no_ins, no_bases, no_rows); });
    run("pile_consensus_pos, calls of another batch", [&] { positions(table, no_call, plan_q, ins, two, rows); });
    run("pile_consensus_pos, device-resident batch", [&] { positions(table, call, plan_q, ins, resident(two), rows); });

    auto segments = [&](const std::vector<uint32_t> &t, const std::vector<uint64_t> &offsets, uint32_t min_len, bool longest) {
        in("table", t), in("offsets", offsets);
        const PileSegments s = pile_segments(t, offsets, 2, 2, min_len, longest, ctx);
        out("segs", s.segs), out("seg_offsets", s.seg_offsets), out("reads", s.reads);
    };
    run("pile_segments", [&] { segments(table, two.offsets, 1, false); });
    run("pile_segments, longest only", [&] { segments(table, two.offsets, 4, true); });
    run("pile_segments, min_len 0", [&] { segments(table, two.offsets, 0, false); });
    run("pile_segments, no read", [&] { segments(no_table, no_reads.offsets, 1, false); });
    run("pile_segments, reads without bases", [&] { segments(no_table, no_bases.offsets, 1, false); });
    run("pile_segments, no offsets", [&] { segments(no_table, {}, 1, false); });
    run("pile_segments, a table of another batch", [&] { segments(no_table, two.offsets, 1, false); });

    const std::vector<uint8_t> bases = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'T'}, none;
    const std::vector<uint64_t> begin = {0, 4}, end = {3, 8}, no_range;
    auto ranges = [&](const std::vector<uint8_t> &s, const std::vector<uint64_t> &b, const std::vector<uint64_t> &e, uint64_t count) {
        in("bases", s), in("begin", b), in("end", e);
        g.count = count;
        out("parts", extract_ranges(s, b, e, ctx));
    };
    run("extract_ranges, 3 bytes", [&] { ranges(bases, begin, end, 3); });
    run("extract_ranges, 0 bytes", [&] { ranges(bases, begin, end, 0); });
    run("extract_ranges, no range", [&] { ranges(bases, no_range, no_range, 0); });
    run("extract_ranges, no base", [&] { ranges(none, begin, begin, 0); });
    run("extract_ranges, more begins than ends", [&] { ranges(bases, begin, no_range, 0); });

    auto corrected = [&](const CorrectedReads &r) { size_of("cons.bases", r.cons.bases), size_of("cons.offsets", r.cons.offsets), size_of("reads", r.reads); };
    run("correct_chains", [&] {
        in("chains", chains), in("b", two);
        corrected(correct_chains(chains, two, 32, 2, 4, ctx));
    });
    run("correct_chains, no chain", [&] { corrected(correct_chains(no_chains, two, 32, 2, 4, ctx)); });
    run("correct_reads", [&] { corrected(correct_reads<Kmer32bit>(two, 5, 3, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, 3, 16, ctx)); });
    run("trim_reads", [&] {
        in("table", table), in("b", two);
        const TrimmedReads t = trim_reads(table, two, 2, 2, 4, false, ctx);
        size_of("out.bases", t.out.bases), size_of("out.offsets", t.out.offsets), size_of("segs", t.segs), size_of("reads", t.reads);
    });
    run("trim_reads, device-resident batch", [&] { trim_reads(table, resident(two), 2, 2, 4, false, ctx); });
    auto trimmed = [&](const CorrectedTrimmedReads &t) {
        size_of("out.bases", t.out.bases), size_of("out.offsets", t.out.offsets), size_of("segs", t.segs), size_of("reads", t.reads), size_of("trims", t.trims);
    };
    run("correct_trim_chains", [&] {
        in("chains", chains), in("b", two);
        trimmed(correct_trim_chains(chains, two, 32, 2, 4, 2, 4, false, ctx));
    });
    run("correct_trim_chains, device-resident batch", [&] { correct_trim_chains(chains, resident(two), 32, 2, 4, 2, 4, false, ctx); });
    run("correct_trim_reads", [&] { trimmed(correct_trim_reads<Kmer32bit>(two, 5, 3, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, 3, 16, 3, 4, true, ctx)); });
}

void graph_cases(Context &ctx) {
    const std::vector<kmu_chain> chains = chains_of(2), no_chains;
    const std::vector<kmu_chain_aln> aln(2, kmu_chain_aln{1, 7, 3, 1}), no_aln;
    const std::vector<uint64_t> offsets = {0, 10, 22}, one = {0}, no_offsets;
    GraphParams gp;
    gp.min_overlap = 5, gp.max_hang = 3, gp.min_identity_permille = 800, gp.fuzz = 2;
    auto classify = [&](const std::vector<kmu_chain> &c, const std::vector<kmu_chain_aln> &a, const std::vector<uint64_t> &o) {
        in("chains", c), in("aln", a), in("offsets", o);
        const OverlapClasses r = sg_classify(c, a, o, gp, ctx);
        out("classes", r.classes), out("reads", r.reads);
    };
    run("sg_classify", [&] { classify(chains, aln, offsets); });
    run("sg_classify, no alignment record", [&] { classify(chains, no_aln, offsets); });
    run("sg_classify, no chain", [&] { classify(no_chains, no_aln, offsets); });
    run("sg_classify, no read", [&] { classify(no_chains, no_aln, one); });
    run("sg_classify, no offsets", [&] { classify(chains, aln, no_offsets); });
    run("sg_classify, records of other chains", [&] { classify(no_chains, aln, offsets); });
    auto graph = [&](const std::vector<kmu_chain> &c, const std::vector<kmu_chain_aln> &a, const std::vector<uint64_t> &o, uint64_t count) {
        in("chains", c), in("aln", a), in("offsets", o);
        g.count = count;
        const OverlapGraph r = overlap_graph(c, a, o, gp, ctx);
        out("arcs", r.arcs), out("arc_offsets", r.arc_offsets), out("classes", r.classes), out("reads", r.reads);
    };
    run("overlap_graph, 3 arcs", [&] { graph(chains, aln, offsets, 3); });
    run("overlap_graph, 0 arcs", [&] { graph(chains, aln, offsets, 0); });
    run("overlap_graph, no alignment record", [&] { graph(chains, no_aln, offsets, 3); });
    run("overlap_graph, no chain", [&] { graph(no_chains, no_aln, offsets, 0); });
    run("overlap_graph, no read", [&] { graph(no_chains, no_aln, one, 0); });
    run("overlap_graph, no offsets", [&] { graph(chains, aln, no_offsets, 0); });
    run("read_graph", [&] {
        const OverlapGraph r = read_graph<Kmer32bit>(ascii(TWO), 5, 3, gp, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, ctx);
        size_of("arcs", r.arcs), size_of("arc_offsets", r.arc_offsets), size_of("classes", r.classes), size_of("reads", r.reads);
    });
    run("read_graph, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO);
        read_graph<Kmer32bit>(resident(host), 5, 3, gp, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, ctx);
    });
    const std::vector<kmu_sg_arc> arcs(3, kmu_sg_arc{0, 2, 5, 5, 0, 0, 1, 0}), no_arcs;
    run("unitig_labels", [&] {
        in("arcs", arcs);
        size_of("labels", unitig_labels(arcs, 2, ctx));
    });
    run("unitig_labels, no arc", [&] { size_of("labels", unitig_labels(no_arcs, 2, ctx)); });
    run("unitig_labels, no read", [&] { size_of("labels", unitig_labels(no_arcs, 0, ctx)); });

    const std::vector<kmu_sg_read> reads(2, kmu_sg_read{0, 1, 1, 0}), no_reads;
    auto unitigs = [&](const std::vector<kmu_sg_arc> &a, const std::vector<kmu_sg_read> &r, const std::vector<uint64_t> &o) {
        in("arcs", a), in("reads", r), in("offsets", o);
        out("layout", sg_unitigs(a, r, o, ctx));
    };
    run("sg_unitigs", [&] { unitigs(arcs, reads, offsets); });
    run("sg_unitigs, no summary", [&] { unitigs(arcs, no_reads, offsets); });
    run("sg_unitigs, no arc", [&] { unitigs(no_arcs, reads, offsets); });
    run("sg_unitigs, no read", [&] { unitigs(no_arcs, no_reads, one); });
    run("sg_unitigs, no offsets", [&] { unitigs(arcs, reads, no_offsets); });
    run("sg_unitigs, summaries of another batch", [&] { unitigs(arcs, reads, one); });
    const std::vector<uint8_t> bases(22, 'A'), no_bases;
    auto sequences = [&](const Unitigs &u, const std::vector<uint8_t> &b, const std::vector<uint64_t> &o, uint64_t count) {
        in("layout", u), in("bases", b), in("offsets", o);
        g.count = count;
        const UnitigSequences s = unitig_sequences(u, b, o, ctx);
        out("seq", s.seq), out("seq_offsets", s.seq_offsets);
    };
    run("unitig_sequences, 3 bases", [&] { sequences(layout_of(2), bases, offsets, 3); });
    run("unitig_sequences, 0 bases", [&] { sequences(layout_of(2), bases, offsets, 0); });
    run("unitig_sequences, no unitig", [&] { sequences(layout_of(0), bases, offsets, 0); });
    run("unitig_sequences, no read", [&] { sequences(layout_of(0), no_bases, one, 0); });
    run("unitig_sequences, no offsets", [&] { sequences(layout_of(2), bases, no_offsets, 0); });
    run("read_unitigs", [&] {
        const ReadUnitigs r = read_unitigs<Kmer32bit>(ascii(TWO), 5, 3, gp, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, ctx);
        size_of("unitigs", r.layout.unitigs), size_of("path", r.layout.path), size_of("place", r.layout.place), size_of("seq", r.sequences.seq),
            size_of("seq_offsets", r.sequences.seq_offsets);
    });
    run("read_unitigs, device-resident batch", [&] {
        const detail::Batch host = ascii(TWO);
        read_unitigs<Kmer32bit>(resident(host), 5, 3, gp, FHash::canon_invhash, 0, 5000, 500, 3, 0, 64, ctx);
    });

    auto clean = [&](const std::vector<kmu_sg_arc> &a, const std::vector<kmu_sg_read> &r, uint32_t n) {
        in("arcs", a), in("reads", r);
        const CleanGraph c = sg_clean(a, r, n, 3, 5, ctx);
        out("arcs", c.arcs), out("reads", c.reads);
        T("n_arcs_left", c.stats.n_arcs_left);
    };
    run("sg_clean", [&] { clean(arcs, reads, 2); });
    run("sg_clean, no summary", [&] { clean(arcs, no_reads, 2); });
    run("sg_clean, no arc", [&] { clean(no_arcs, reads, 2); });
    run("sg_clean, no read", [&] { clean(no_arcs, no_reads, 0); });
    run("sg_clean, summaries of another batch", [&] { clean(arcs, reads, 3); });
    run("clean_graph, 2 rounds", [&] {
        const CleanGraph c = clean_graph(arcs, reads, 2, 3, 5, 2, ctx);
        size_of("arcs", c.arcs), size_of("reads", c.reads);
        T("n_tip_reads", c.stats.n_tip_reads);
    });
    run("clean_graph, a round that removes nothing", [&] {
        g.count = 0;
        const CleanGraph c = clean_graph(arcs, reads, 2, 3, 5, 4, ctx);
        size_of("arcs", c.arcs), size_of("reads", c.reads);
    });
    run("clean_graph, no round", [&] { size_of("arcs", clean_graph(arcs, reads, 2, 3, 5, 0, ctx).arcs); });

    const std::vector<uint8_t> classes(2, 1), no_classes;
    auto map = [&](const Unitigs &u, const std::vector<kmu_chain> &c, const std::vector<uint8_t> &cl, const std::vector<uint64_t> &o, bool alias = false) {
        in("layout", u), in("chains", c), in("classes", cl), in("offsets", o);
        const UnitigChains r = alias ? unitig_read_chains(u, c, cl, o, ctx) : sg_unitig_chains(u, c, cl, o, ctx);
        out("records", r.records);
    };
    run("sg_unitig_chains", [&] { map(layout_of(2), chains, classes, offsets); });
    run("sg_unitig_chains, no chain", [&] { map(layout_of(2), no_chains, no_classes, offsets); });
    run("sg_unitig_chains, one record", [&] {
        g.count = 1;
        map(layout_of(2), chains, classes, offsets);
    });
    run("sg_unitig_chains, no read", [&] { map(layout_of(0), no_chains, no_classes, one); });
    run("sg_unitig_chains, no offsets", [&] { map(layout_of(2), chains, classes, no_offsets); });
    run("sg_unitig_chains, places of another batch", [&] { map(layout_of(0), chains, classes, offsets); });
    run("sg_unitig_chains, classes of other chains", [&] { map(layout_of(2), chains, no_classes, offsets); });
    run("unitig_read_chains", [&] { map(layout_of(2), chains, classes, offsets, true); });
    auto polished = [&](const PolishedUnitigs &p) {
        size_of("cons.bases", p.cons.bases), size_of("cons.offsets", p.cons.offsets), size_of("unitigs", p.layout.unitigs), size_of("path", p.layout.path),
            size_of("summaries", p.summaries), size_of("records", p.records), size_of("aln", p.aln);
    };
    UnitigSequences seqs;
    seqs.seq.assign(12, 'C');
    seqs.seq_offsets = {0, 12};
    run("polish_unitigs", [&] { polished(polish_unitigs(layout_of(2), seqs, ascii(TWO), chains, classes, 32, 0, 2, 4, 1, ctx)); });
    run("polish_unitigs, 2 rounds, no chain", [&] { polished(polish_unitigs(layout_of(2), seqs, ascii(TWO), {}, {}, 32, 0, 2, 4, 2, ctx)); });
    run("polish_unitigs, device-resident reads", [&] {
        const detail::Batch host = ascii(TWO);
        polish_unitigs(layout_of(2), seqs, resident(host), {}, {}, 32, 0, 2, 4, 1, ctx);
    });
}

void counting_cases(Context &ctx) {
    const std::vector<Sequence> seqs = {Sequence("ACGTACGTAC"), Sequence("GGCATTGCAGTA")};
    const detail::Batch two = ascii(TWO), no_reads = ascii({});
    run("KmerCounter: single k-mers", [&] {
        KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
        T("distinct before the first insertion", c.get_nb_distinct());
        T("unique before the first insertion", c.get_nb_unique());
        c.eliminate_once_kmer();
        size_of("above2 before the first insertion", c.above2_entries().first);
        c.insert_kmer(Kmer32bit::build(5, 3));
        c.insert_kmer(Kmer32bit::build(9, 3));
        T("count", c.get_count(Kmer32bit::build(5, 3)));
        T("distinct", c.get_nb_distinct());
        T("unique", c.get_nb_unique());
        T("above2", c.get_above2_count(Kmer32bit::build(5, 3)));
        size_of("counts", c.get_count(std::vector<Kmer32bit>{Kmer32bit::build(5, 3), Kmer32bit::build(6, 3)}));
        size_of("no counts", c.get_count(std::vector<Kmer32bit>{}));
        c.eliminate_once_kmer();
        size_of("histogram", c.get_count_histogram());
        c.insert_kmer(Kmer32bit::build(7, 3));
        T("raw flushes", int(c.raw() != nullptr));
    });
    run("KmerCounter::insert_reads", [&] {
        KmerCounter<Kmer64bit> c(0.03, 1000, 4, ctx);
        size_of("histogram before the first insertion", c.get_count_histogram());
        in("two", two);
        c.insert_reads(two, 5);
        c.insert_reads(detail::pointers(seqs), 5);
        c.insert_reads(no_reads, 5);
        const detail::Batch dev = resident(two);
        c.insert_reads(dev, 5);
    });
    for (uint64_t count : {3, 0})
        run(count ? "KmerCounter::above2_entries, 3 entries" : "KmerCounter::above2_entries, 0 entries", [&] {
            KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
            c.insert_reads(two, 5);
            g.count = count;
            const auto e = c.above2_entries();
            out("kmers", e.first), out("counts", e.second);
        });
    run("KmerCounterPool::above2_entries", [&] {
        KmerCounterPool<Kmer32bit> pool(1000, 8, ctx);
        pool.counter().insert_reads(two, 5);
        size_of("kmers", pool.above2_entries().first);
    });
    auto abundance = [&](const detail::Batch &b, bool inserted) {
        KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
        if (inserted) c.insert_reads(two, 5);
        in("b", b);
        const auto r = c.get_reads_abundance(b, 3);
        out("counts", r.counts), out("stats", r.stats);
    };
    run("KmerCounter::get_reads_abundance", [&] { abundance(ascii(TWO_DB), true); });
    run("KmerCounter::get_reads_abundance, packed sequences", [&] {
        KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
        c.insert_reads(two, 5);
        const auto r = c.get_reads_abundance(detail::pointers(seqs));
        out("counts", r.counts), out("stats", r.stats);
    });
    run("KmerCounter::get_reads_abundance, no read", [&] { abundance(no_reads, true); });
    run("KmerCounter::get_reads_abundance, reads without bases", [&] { abundance(ascii(NO_BASES), true); });
    run("KmerCounter::get_reads_abundance, nothing inserted", [&] { abundance(two, false); });
    run("KmerCounter::get_reads_abundance, device-resident batch", [&] { abundance(resident(two), true); });

    auto once = [&](const detail::Batch &b, uint64_t count, bool inserted = true) {
        KmerFilter1 f(16, 1000, ctx);
        if (inserted) f.insert_reads(two);
        T("once", f.get_nb_once());
        in("b", b);
        g.count = count;
        const KmerFilter1::OnceKmers r = f.once_positions(b);
        out("kmin", r.kmin), out("numseq", r.numseq), out("numkmer", r.numkmer);
    };
    run("KmerFilter1::once_positions, 3 k-mers", [&] { once(two, 3); });
    run("KmerFilter1::once_positions, 0 k-mers", [&] { once(two, 0); });
    run("KmerFilter1::once_positions, packed sequences", [&] { once(detail::gather(detail::pointers(seqs)), 3); });
    run("KmerFilter1::once_positions, device-resident batch, 3 k-mers", [&] { once(resident(two), 3); });
    run("KmerFilter1::once_positions, device-resident batch, 0 k-mers", [&] { once(resident(two), 0); });
    run("KmerFilter1::once_positions, nothing inserted", [&] { once(two, 3, false); });
    run("KmerFilter1 of 15-mers", [&] { KmerFilter1 f(15, 1000, ctx); });
    run("KmerFilter1::insert_kmer16b32bit", [&] {
        KmerFilter1 f(16, 1000, ctx);
        f.insert_kmer16b32bit(Kmer16b32bit(77));
        T("once", f.get_nb_once());
    });
    run("filter1_kmer_16b32bit", [&] { T("once", filter1_kmer_16b32bit(seqs, ctx)->get_nb_once()); });
    run("count_kmer_threaded_one_to_many", [&] { T("distinct", count_kmer_threaded_one_to_many<Kmer32bit>(seqs, 2, 8, 5, ctx)->get_nb_distinct()); });
    run("count_kmer_thread_independant", [&] { T("distinct", count_kmer_thread_independant<Kmer64bit>(seqs, 2, 17, ctx)->get_nb_distinct()); });
    run("count_kmer16b32bit", [&] { T("distinct", count_kmer16b32bit(seqs, ctx)->get_nb_distinct()); });
    run("count_kmer32bit", [&] { T("distinct", count_kmer32bit(seqs, 11, ctx)->get_nb_distinct()); });
    run("count_kmer32bit, k = 15", [&] { count_kmer32bit(seqs, 15, ctx); });
    run("count_kmer64bit", [&] { T("distinct", count_kmer64bit(seqs, 21, ctx)->get_nb_distinct()); });
    run("count_kmer64bit, k = 16", [&] { count_kmer64bit(seqs, 16, ctx); });
    run("count_kmer64bit, k = 33", [&] { count_kmer64bit(seqs, 33, ctx); });

    run("KmerPrefilter", [&] {
        T("cells", KmerPrefilter<Kmer32bit>::cells_for(100, 16));
        KmerPrefilter<Kmer32bit> f(5, 64, 3, ctx), other(5, 64, 3, ctx);
        in("two", two);
        f.insert_reads(two);
        f.insert_reads(detail::pointers(seqs));
        const detail::Batch dev = resident(two);
        f.insert_reads(dev);
        f.insert_reads(no_reads);
        f.insert_kmer(Kmer32bit::build(5, 5));
        f.insert_kmer(std::vector<Kmer32bit>{});
        T("class", f.seen_class(Kmer32bit::build(5, 5)));
        size_of("classes", f.seen_class(std::vector<Kmer32bit>{Kmer32bit::build(5, 5), Kmer32bit::build(6, 5)}));
        size_of("no classes", f.seen_class(std::vector<Kmer32bit>{}));
        T("n_cells", f.info().n_cells);
        f.merge(other);
        const std::vector<uint64_t> w = f.words();
        out("words", w);
        T("passing", f.nb_passing(two));
        T("passing on the device", f.nb_passing(dev));
        KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
        T("passed", c.insert_reads_filtered(f, two, 5));
        T("passed, packed", c.insert_reads_filtered(f, detail::gather(detail::pointers(seqs)), 5));
        T("passed on the device", c.insert_reads_filtered(f, dev, 5));
    });
    run("KmerPrefilter::cells_for, too many cells", [&] {
        g.cells = 0;
        KmerPrefilter<Kmer32bit>::cells_for(uint64_t(1) << 40, 16);
    });
    run("KmerPrefilter, the library refuses", [&] {
        g.fail = KMU_E_BAD_ARG;
        KmerPrefilter<Kmer32bit> f(5, 0, 3, ctx);
    });
    run("count_repeated_kmers", [&] {
        in("two", two);
        const RepeatedKmers<Kmer32bit> r = count_repeated_kmers<Kmer32bit>(two, 5, 8, 16, 4, 0, ctx);
        T("nb_passed", r.nb_passed);
    });
    run("count_repeated_kmers of sequences, with a capacity", [&] { T("nb_passed", count_repeated_kmers<Kmer32bit>(seqs, 5, 8, 12, 3, 5000, ctx).nb_passed); });
    run("count_repeated_kmers, no read", [&] { T("nb_passed", count_repeated_kmers<Kmer32bit>(no_reads, 5, 8, 16, 4, 0, ctx).nb_passed); });
}

void io_cases(Context &ctx, const std::string &tmp) {
    const std::string text = "@r0\nACGTACGTAC\n+\nIIIIIIIIII\n@r1\nGGCATTGCAG\n+\nIIIIIIIIII\n";
    const std::vector<uint8_t> bytes(text.begin(), text.end());
    auto parsed = [&](uint64_t count) {
        in("text", bytes);
        g.count = count;
        const FastqReads r = parse_fastx_text(bytes.data(), bytes.size(), ctx);
        out("bases", r.bases), out("offsets", r.offsets);
    };
    run("parse_fastx_text", [&] { parsed(2); });
    run("parse_fastx_text, no record kept", [&] { parsed(0); });
    run("parse_fastq_text", [&] {
        in("text", bytes);
        size_of("offsets", parse_fastq_text(bytes.data(), bytes.size(), ctx).offsets);
    });
    run("DeviceReads::from_device_text and batch", [&] {
        in("text", bytes);
        g.count = 2;
        const DeviceReads r = DeviceReads::from_device_text(ctx, bytes.data(), bytes.size());
        out("offsets", r.offsets);
        const detail::Batch all = r.batch(0, 2), second = r.batch(1, 2);
        size_of("all.offsets", all.offsets), size_of("second.offsets", second.offsets);
        KmerCounter<Kmer32bit> c(0.03, 1000, 8, ctx);
        c.insert_reads(all, 5);
        c.insert_reads(second, 5);
    });
    run("DeviceReads::from_file, parse_fastq_file", [&] {
        const std::string fname = tmp + "/marshal_reads.fq";
        FILE *f = fopen(fname.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot write " + fname);
        fwrite(text.data(), 1, text.size(), f);
        fclose(f);
        g.count = 2;
        size_of("device offsets", DeviceReads::from_file(fname, ctx, 16, 1).offsets);
        g.count = 2;
        size_of("host offsets", parse_fastq_file(fname, ctx).offsets);
        remove(fname.c_str());
    });
    run("DeviceReads::from_file, no such file", [&] { DeviceReads::from_file("no_such_dir/no_such_file.fq", ctx); });
}

}  // namespace

int main(int argc, char **argv) {
    const std::string tmp = argc > 1 ? argv[1] : "/tmp";
    Context ctx(0);
    sketch_cases(ctx);
    signature_cases(ctx);
    block_and_bottomk_cases(ctx);
    anchor_cases(ctx);
    component_cases(ctx);
    minimizer_cases(ctx);
    chain_cases(ctx);
    correction_cases(ctx);
    graph_cases(ctx);
    counting_cases(ctx);
    io_cases(ctx, tmp);
    fprintf(stderr, "%zu cases, %zu lines\n", g_n_cases, g_n_lines);
    return 0;
}

"""-m "not gpu": the string graph without a device.  The references that the device tests compare against -- reference_classify and
reference_graph, sets and loops straight from the contract in include/kmu.h, and reference_myers, the sequential transitive
reduction with its in-play skip -- the hand cases and the planted layouts that make them trustworthy, and the refusals the library
makes before it launches anything."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from kmerutils_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN, ALN = np.dtype(A.CHAIN_DTYPE), np.dtype(A.CHAIN_ALN_DTYPE)
ARC, READ = np.dtype(A.SG_ARC_DTYPE), np.dtype(A.SG_READ_DTYPE)
PARAMS = dict(min_overlap=50, max_hang=1000, int_permille=250, min_identity_permille=0, fuzz=0)


class Refused(Exception):
    """the call is KMU_E_UNSUPPORTED: a record fault"""


def params(**kw):
    p = dict(PARAMS)
    p.update(kw)
    return p


def rec(a, b, s, a_start, a_end, b_start, b_end):
    """one chain record; score and the seed counts play no part in the graph"""
    return (a, b, s, 0, 0, 0, a_start, a_end, b_start, b_end)


def records(rows):
    return np.array([rec(*r) for r in rows], CHAIN) if len(rows) else np.zeros(0, CHAIN)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.uint64))]).astype(np.uint64)


def hangs(r, la, lb):
    a_start, a_end, b_start, b_end, s = int(r["a_start"]), int(r["a_end"]), int(r["b_start"]), int(r["b_end"]), int(r["strand"])
    bs, be = (b_start, b_end) if s == 0 else (lb - b_end, lb - b_start)
    return a_start, la - a_end, bs, lb - be


def reference_classify(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz=0):
    """(classes, reads) of the contract; Refused for a record fault.  The degrees of the summaries stay 0."""
    off = [int(x) for x in offsets]
    n_reads = len(off) - 1
    classes = np.zeros(len(chains), np.uint8)
    reads = np.zeros(n_reads, READ)
    for r in chains:
        a, b = int(r["read_a"]), int(r["read_b"])
        if a >= n_reads or b >= n_reads or int(r["strand"]) > 1 or r["a_start"] > r["a_end"] or r["b_start"] > r["b_end"]:
            raise Refused
        if r["a_end"] > off[a + 1] - off[a] or r["b_end"] > off[b + 1] - off[b] or max(off[a + 1] - off[a], off[b + 1] - off[b]) >= 1 << 32:
            raise Refused
    for c, r in enumerate(chains):
        a, b = int(r["read_a"]), int(r["read_b"])
        la, lb = off[a + 1] - off[a], off[b + 1] - off[b]
        oa, ob = int(r["a_end"]) - int(r["a_start"]), int(r["b_end"]) - int(r["b_start"])
        aL, aR, bL, bR = hangs(r, la, lb)
        hang, maplen = min(aL, bL) + min(aR, bR), max(oa, ob)
        if a >= b:
            cls = A.SG_SKIP
        elif oa < min_overlap or ob < min_overlap:
            cls = A.SG_SHORT
        elif aln is not None and (not int(aln[c]["flags"]) & A.ALN_DONE or int(aln[c]["matches"]) * 1000 < min_identity_permille * (
                int(aln[c]["matches"]) + int(aln[c]["edit"]))):
            cls = A.SG_LOWID
        elif hang > max_hang or hang * 1000 > maplen * int_permille:
            cls = A.SG_INTERNAL
        else:
            a_in, b_in = aL <= bL and aR <= bR, aL >= bL and aR >= bR
            if a_in and b_in:
                cls = A.SG_A_CONTAINED if la < lb else A.SG_B_CONTAINED
            elif a_in:
                cls = A.SG_A_CONTAINED
            elif b_in:
                cls = A.SG_B_CONTAINED
            else:
                cls = A.SG_DOVETAIL
        classes[c] = cls
        if cls != A.SG_SKIP:
            reads["n_records"][a] += 1
            reads["n_records"][b] += 1
        if cls == A.SG_A_CONTAINED:
            reads["flags"][a] |= A.SG_READ_CONTAINED
        if cls == A.SG_B_CONTAINED:
            reads["flags"][b] |= A.SG_READ_CONTAINED
    return classes, reads


def reference_arcs(chains, classes, reads, offsets):
    """the arcs (from, to, len, ovl, rec) of the contract in (from, to, rec) order"""
    off = [int(x) for x in offsets]
    arcs = []
    for c, r in enumerate(chains):
        a, b, s = int(r["read_a"]), int(r["read_b"]), int(r["strand"])
        if classes[c] != A.SG_DOVETAIL or reads["flags"][a] & A.SG_READ_CONTAINED or reads["flags"][b] & A.SG_READ_CONTAINED:
            continue
        aL, aR, bL, bR = hangs(r, off[a + 1] - off[a], off[b + 1] - off[b])
        oa, ob = int(r["a_end"]) - int(r["a_start"]), int(r["b_end"]) - int(r["b_start"])
        if aL > bL:
            arcs += [(2 * a, 2 * b + s, bR - aR, oa, c), (2 * b + (s ^ 1), 2 * a + 1, aL - bL, ob, c)]
        else:
            arcs += [(2 * a + 1, 2 * b + (s ^ 1), bL - aL, oa, c), (2 * b + s, 2 * a, aR - bR, ob, c)]
        assert aL != bL and arcs[-1][2] >= 1 and arcs[-2][2] >= 1
    return sorted(arcs, key=lambda x: (x[0], x[1], x[4]))


def out_lists(arcs):
    out = {}
    for i, x in enumerate(arcs):
        out.setdefault(x[0], []).append(i)
    return out


def reference_marks(arcs, fuzz):
    """the records the contract's rule marks: for every f = v -> w and g = w -> x that satisfy it, every arc v -> x"""
    out = out_lists(arcs)
    marked = set()
    for v, ov in out.items():
        limit = max(arcs[i][2] for i in ov) + fuzz
        to_x = {}
        for i in ov:
            to_x.setdefault(arcs[i][1], []).append(arcs[i][4])
        for i in ov:
            len_f, ow = arcs[i][2], out.get(arcs[i][1], [])
            if not ow:
                continue
            first = min(ow, key=lambda j: (arcs[j][2], arcs[j][1], arcs[j][4]))
            for j in ow:
                if len_f + arcs[j][2] <= limit or arcs[j][2] < fuzz or j == first:
                    marked.update(to_x.get(arcs[j][1], ()))
    return marked


def reference_myers(arcs, fuzz):
    """Myers' sequential transitive reduction (2005) on the same arcs: the records of the arcs it removes, mates included.  Unlike the
    contract's rule it looks through w only while w is still in play, and it walks out(w) in order of length and stops early."""
    out = out_lists(arcs)
    by_len = {v: sorted(ov, key=lambda i: (arcs[i][2], arcs[i][1], arcs[i][4])) for v, ov in out.items()}
    vacant, inplay, eliminated = 0, 1, 2
    removed = set()
    for v, ov in by_len.items():
        mark = {arcs[i][1]: inplay for i in ov}
        limit = arcs[ov[-1]][2] + fuzz
        for i in ov:
            w = arcs[i][1]
            if mark[w] != inplay:
                continue
            for j in by_len.get(w, []):
                if arcs[i][2] + arcs[j][2] > limit:
                    break
                if mark.get(arcs[j][1], vacant) == inplay:
                    mark[arcs[j][1]] = eliminated
        for i in ov:
            for n, j in enumerate(by_len.get(arcs[i][1], [])):
                if n > 0 and arcs[j][2] >= fuzz:
                    break
                if mark.get(arcs[j][1], vacant) == inplay:
                    mark[arcs[j][1]] = eliminated
        removed.update(arcs[i][4] for i in ov if mark[arcs[i][1]] == eliminated)
    return removed


def reference_graph(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille, fuzz):
    """(arcs, arc_offsets, classes, reads) of the contract"""
    classes, reads = reference_classify(chains, aln, offsets, min_overlap, max_hang, int_permille, min_identity_permille)
    n_reads = len(offsets) - 1
    arcs = reference_arcs(chains, classes, reads, offsets)
    marked = reference_marks(arcs, fuzz)
    res = np.zeros(len(arcs), ARC)
    for i, (v, t, ln, ovl, c) in enumerate(arcs):
        res[i] = (v, t, ln, ovl, c, A.SG_ARC_REDUCED if c in marked else 0, 0, 0)
    out = out_lists(arcs)
    alive = {v: [i for i in out.get(v, []) if not res["flags"][i]] for v in range(2 * n_reads)}
    for v in range(2 * n_reads):
        reads["out_rev" if v & 1 else "out_fwd"][v >> 1] = len(alive[v])
    by_rec = {}
    for j, x in enumerate(arcs):
        by_rec.setdefault(x[4], []).append(j)
    for i, (v, t, ln, ovl, c) in enumerate(arcs):
        if res["flags"][i]:
            continue
        mate, = [j for j in by_rec[c] if j != i]  # a record makes exactly two arcs
        assert arcs[mate][0] == t ^ 1 and arcs[mate][1] == v ^ 1
        res["unique"][i] = 1 if alive[v] == [i] and alive[t ^ 1] == [mate] else 0
    arc_offsets = np.zeros(2 * n_reads + 1, np.uint64)
    for v, _, _, _, _ in arcs:
        arc_offsets[v + 1:] += 1
    return res, arc_offsets, classes, reads


# ---- planted layouts: reads cut from one line, so the truth is known without the code -------------------------------------------
def layout_records(starts, lengths, seed, jitter=0, min_share=50, doubled=0.0, perturb=0):
    """Reads [start, start + length) of one line with random strands, shuffled ids and shuffled records: one record for every pair
    that shares at least min_share bases, the smaller id as read_a.  jitter: every coordinate moves by up to that much (inside its
    read); perturb: the hostile variant, a hang moves by up to that much; doubled: the share of records written twice.  Returns
    (chains, offsets, ids) -- ids[i] is the read id of line read i."""
    rng = np.random.default_rng(seed)
    n = len(starts)
    ids = rng.permutation(n)
    flip = rng.integers(0, 2, n)
    lengths_by_id = np.zeros(n, np.int64)
    lengths_by_id[ids] = lengths
    rows = []

    def on_read(i, lo, hi):  # the line interval [lo, hi) in the coordinates of read i as it is stored
        s, e = starts[i], starts[i] + lengths[i]
        return (e - hi, e - lo) if flip[i] else (lo - s, hi - s)

    def moved(x, length, by):
        return int(min(max(x + rng.integers(-by, by + 1), 0), length)) if by else int(x)

    for i in range(n):
        for j in range(i + 1, n):
            lo, hi = max(starts[i], starts[j]), min(starts[i] + lengths[i], starts[j] + lengths[j])
            if hi - lo < min_share:
                continue
            a, b = (i, j) if ids[i] < ids[j] else (j, i)
            (a0, a1), (b0, b1) = on_read(a, lo, hi), on_read(b, lo, hi)
            by = max(jitter, perturb)
            a0, b0 = moved(a0, lengths[a], by), moved(b0, lengths[b], by)
            a1, b1 = max(moved(a1, lengths[a], by), a0), max(moved(b1, lengths[b], by), b0)
            row = (int(ids[a]), int(ids[b]), int(flip[a] ^ flip[b]), a0, a1, b0, b1)
            rows.append(row)
            if rng.random() < doubled:
                rows.append(row)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    return records(rows), offsets_of(lengths_by_id), ids


@functools.lru_cache(maxsize=None)
def planted_tiling(jitter):
    """(i): 27 reads of 400 at step 100 over 3 000 bases; exact, or every coordinate jittered by up to 3 at fuzz 10"""
    chains, offsets, ids = layout_records(np.arange(27) * 100, np.full(27, 400), seed=11 + jitter, jitter=jitter)
    return chains, offsets, ids, params(fuzz=10 if jitter else 0)


@functools.lru_cache(maxsize=None)
def planted_random():
    """(ii): 120 reads of 150 .. 600 bases at random starts over 4 000"""
    rng = np.random.default_rng(5)
    lengths = rng.integers(150, 601, 120)
    starts = np.array([rng.integers(0, 4000 - ln + 1) for ln in lengths])
    chains, offsets, ids = layout_records(starts, lengths, seed=6)
    return chains, offsets, ids, params(), starts, lengths


@functools.lru_cache(maxsize=None)
def planted_pile(n):
    """(iii): n reads of 400 at step 2 -- every read overlaps every other, the largest out-degree is n - 1"""
    chains, offsets, ids = layout_records(np.arange(n) * 2, np.full(n, 400), seed=100 + n)
    return chains, offsets, ids, params()


@functools.lru_cache(maxsize=None)
def planted_reference(name, arg=None):
    """reference_graph of a planted layout, computed once for every test that needs it (device tests included)"""
    case = {"tiling": planted_tiling, "random": planted_random, "pile": planted_pile}[name]
    got = case(arg) if arg is not None else case()
    return reference_graph(got[0], None, got[1], **got[3])


def arc_tuples(arcs):
    return [tuple(int(v) for v in x)[:5] for x in arcs.tolist()]


def reduced_records(arcs):
    return set(int(c) for c in arcs["rec"][arcs["flags"] != 0])


def out_degrees(reads):
    return np.stack([reads["out_fwd"], reads["out_rev"]], axis=1).reshape(-1)


def host_components(n_nodes, edges):
    label = list(range(n_nodes))

    def find(x):
        while label[x] != x:
            label[x] = label[label[x]]
            x = label[x]
        return x
    for u, v in edges:
        ru, rv = find(u), find(v)
        if ru != rv:
            label[max(ru, rv)] = min(ru, rv)
    return [find(x) for x in range(n_nodes)]


# ---- hand cases, worked out on paper -------------------------------------------------------------------------------------------
# reads 0 .. 3 have 1 000 bases each unless a case says otherwise
def test_each_of_the_six_classes():
    off = offsets_of([1000, 1000, 1000, 300])
    aln = np.zeros(7, ALN)
    aln["flags"], aln["matches"], aln["edit"] = A.ALN_DONE, 900, 100
    aln[2] = (0xFFFFFFFF, 0, 2000, 0)  # not DONE
    chains = records([
        (1, 0, 0, 600, 1000, 0, 400),    # read_a >= read_b                                   SKIP
        (0, 1, 0, 960, 1000, 0, 40),     # 40 < min_overlap 50                                SHORT
        (0, 1, 0, 600, 1000, 0, 400),    # a dovetail, but its alignment was not done         LOWID
        (0, 1, 0, 300, 700, 300, 700),   # hang 300 + 300 on 400 bases                        INTERNAL
        (0, 3, 0, 200, 500, 0, 300),     # read 3 (300 bases) lies inside read 0              B_CONTAINED
        (3, 0, 0, 0, 300, 200, 500),     # SKIP by order: the same pair from the other side
        (0, 1, 0, 600, 1000, 0, 400),    # aL 600 > bL 0, aR 0 < bR 600                       DOVETAIL
    ])
    classes, reads = reference_classify(chains, aln, off, **params(min_identity_permille=900))
    assert classes.tolist() == [A.SG_SKIP, A.SG_SHORT, A.SG_LOWID, A.SG_INTERNAL, A.SG_B_CONTAINED, A.SG_SKIP, A.SG_DOVETAIL]
    assert reads["flags"].tolist() == [0, 0, 0, A.SG_READ_CONTAINED]
    assert reads["n_records"].tolist() == [5, 4, 0, 1]
    # identity exactly at the bound passes, one edit more does not
    aln[6] = (101, 900, 9, A.ALN_DONE)
    assert reference_classify(chains, aln, off, **params(min_identity_permille=900))[0][6] == A.SG_LOWID
    # A_CONTAINED: read 3 as read_a of a record with a longer read
    off2 = offsets_of([300, 1000])
    assert reference_classify(records([(0, 1, 1, 0, 300, 100, 400)]), None, off2, **params())[0].tolist() == [A.SG_A_CONTAINED]


def test_the_four_dovetails_and_their_arcs():
    off = offsets_of([1000, 800])
    want = {
        # a's right end meets b's left end, same strand:   a+ -> b+ by bR - aR = 500, mate b- -> a- by aL - bL = 700
        (0, 700, 1000, 0, 300): [(0, 2, 500, 300, 0), (3, 1, 700, 300, 0)],
        # b's right end meets a's left end, same strand:   a- -> b- by bL - aL = 550, mate b+ -> a+ by aR - bR = 750
        (0, 0, 250, 550, 800): [(1, 3, 550, 250, 0), (2, 0, 750, 250, 0)],
        # a's right end meets b's right end, opposite:     b forward [500, 800) is bL = 0, bR = 500 in a's orientation
        (1, 700, 1000, 500, 800): [(0, 3, 500, 300, 0), (2, 1, 700, 300, 0)],
        # a's left end meets b's left end, opposite:       b forward [0, 250) is bL = 550, bR = 0
        (1, 0, 250, 0, 250): [(1, 2, 550, 250, 0), (3, 0, 750, 250, 0)],
    }
    for (s, a0, a1, b0, b1), arcs in want.items():
        got, arc_off, classes, reads = reference_graph(records([(0, 1, s, a0, a1, b0, b1)]), None, off, **params())
        assert classes.tolist() == [A.SG_DOVETAIL]
        assert arc_tuples(got) == sorted(arcs)
        assert got["flags"].tolist() == [0, 0] and got["unique"].tolist() == [1, 1]
        assert sorted(out_degrees(reads).tolist()) == [0, 0, 1, 1]
        assert arc_off[-1] == 2 and all(arc_off[v + 1] - arc_off[v] == sum(1 for x in arcs if x[0] == v) for v in range(4))


def test_containment_ties_and_chains():
    # both conditions hold (aL = bL and aR = bR) at equal length: read_b is the contained one
    assert reference_classify(records([(0, 1, 0, 0, 500, 0, 500)]), None, offsets_of([500, 500]), **params())[0].tolist() == [A.SG_B_CONTAINED]
    # the same hangs (10 on every side) on reads of 500 and 520 bases -- the aligned parts differ by 20 bases of gaps: the shorter
    # read is the contained one, whichever side it is on
    classes, reads = reference_classify(records([(0, 1, 0, 10, 490, 10, 510)]), None, offsets_of([500, 520]), **params())
    assert classes.tolist() == [A.SG_A_CONTAINED] and reads["flags"].tolist() == [1, 0]
    classes, reads = reference_classify(records([(0, 1, 0, 10, 510, 10, 490)]), None, offsets_of([520, 500]), **params())
    assert classes.tolist() == [A.SG_B_CONTAINED] and reads["flags"].tolist() == [0, 1]
    # a chain 0 c 1 c 2 and a dovetail of read 2 with read 3: reads 0 and 1 are contained, the dovetails of read 1 make no arcs
    off = offsets_of([200, 400, 1000, 1000])
    chains = records([(0, 1, 0, 0, 200, 100, 300), (1, 2, 0, 0, 400, 300, 700), (2, 3, 0, 600, 1000, 0, 400), (1, 3, 0, 300, 400, 0, 100)])
    arcs, _, classes, reads = reference_graph(chains, None, off, **params())
    assert classes.tolist() == [A.SG_A_CONTAINED, A.SG_A_CONTAINED, A.SG_DOVETAIL, A.SG_DOVETAIL]
    assert reads["flags"].tolist() == [1, 1, 0, 0]
    assert arc_tuples(arcs) == [(4, 6, 600, 400, 2), (7, 5, 600, 400, 2)]


def test_hang_bounds_at_equality():
    off = offsets_of([2000, 2000])
    # aL = 1400, bL = 100 + d, aR = 0, bR = 1400 - d: hang = 100 + d on an overlap of 600 / 500 bases
    def cls(b0, **kw):
        return int(reference_classify(records([(0, 1, 0, 1400, 2000, b0, b0 + 500)]), None, off, **params(**kw))[0][0])
    assert cls(100, max_hang=100, int_permille=1000) == A.SG_DOVETAIL
    assert cls(101, max_hang=100, int_permille=1000) == A.SG_INTERNAL
    # hang * 1000 > maplen * int_permille with maplen = max(600, 500) = 600: hang 150 at 250 is 150 000 > 150 000: no
    assert cls(150, max_hang=1000, int_permille=250) == A.SG_DOVETAIL
    assert cls(151, max_hang=1000, int_permille=250) == A.SG_INTERNAL
    assert cls(0, max_hang=0, int_permille=0) == A.SG_DOVETAIL   # no hang at all passes every bound


def line_arcs(lens_from_v, extra):
    """arcs on forward vertices only, as (from, to, len, ovl, rec) with rec = position; no mates: the rule is tested on the arc set"""
    return sorted([(v, t, ln, 0, i) for i, (v, t, ln) in enumerate(lens_from_v + extra)], key=lambda x: (x[0], x[1], x[4]))


def test_rule_bounds_at_equality():
    # v = 0 -> w = 2 (100), v -> x = 4 (300); w -> x (g).  w also has a shorter arc to 6, so g is not first(w)
    for len_g, fuzz, marked in ((200, 0, True), (201, 0, False), (210, 10, True), (211, 10, False)):
        arcs = line_arcs([(0, 2, 100), (0, 4, 300)], [(2, 4, len_g), (2, 6, 50)])
        assert (1 in reference_marks(arcs, fuzz)) == marked, (len_g, fuzz)
        assert (1 in reference_myers(arcs, fuzz)) == marked, (len_g, fuzz)
    # len(g) < fuzz: with f the longest arc of v, len(f) + len(g) <= L(v) says the same up to len(g) == fuzz -- in the contract's rule
    # the clause never fires alone (it does in the sequential algorithm, where w may be out of play) -- so fuzz - 1 and fuzz mark,
    # fuzz + 1 does not
    for len_g, marked in ((9, True), (10, True), (11, False)):
        arcs = line_arcs([(0, 2, 100), (0, 4, 20)], [(2, 4, len_g), (2, 6, 5)])
        assert (1 in reference_marks(arcs, 10)) == marked
    # first(w) alone: the sum is over L and g is long, but g is the smallest arc of w
    arcs = line_arcs([(0, 2, 100), (0, 4, 120)], [(2, 4, 500), (2, 6, 501)])
    assert reference_marks(arcs, 0) == {1} and reference_myers(arcs, 0) == {1}
    arcs = line_arcs([(0, 2, 100), (0, 4, 120)], [(2, 4, 500), (2, 6, 499)])
    assert reference_marks(arcs, 0) == set()
    # every arc v -> x of a run is marked: two records give the same arc
    arcs = line_arcs([(0, 2, 100), (0, 4, 300), (0, 4, 300)], [(2, 4, 200)])
    assert reference_marks(arcs, 0) == {1, 2}


# ---- planted layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 3])
def test_planted_tiling(jitter):
    chains, offsets, ids, p = planted_tiling(jitter)
    arcs, arc_off, classes, reads = planted_reference("tiling", jitter)
    assert len(chains) == 75 and (classes == A.SG_DOVETAIL).all() and not reads["flags"].any()
    assert len(arcs) == 150 and len(reduced_records(arcs)) == 49 and int((arcs["flags"] == 0).sum()) == 52
    deg = out_degrees(reads)
    assert sorted(deg.tolist()) == [0, 0] + [1] * 52
    # the survivors join neighbours on the line
    line = {int(r): i for i, r in enumerate(ids)}
    assert all(abs(line[int(x["from"]) >> 1] - line[int(x["to"]) >> 1]) == 1 for x in arcs[arcs["flags"] == 0])
    assert int(arcs["unique"].sum()) == 52
    labels = host_components(54, [(int(x["from"]), int(x["to"])) for x in arcs if x["unique"]])
    assert len(set(labels)) == 2 and all(labels[2 * r] != labels[2 * r + 1] for r in range(27))
    assert reduced_records(arcs) == reference_myers(arc_tuples(arcs), p["fuzz"])


def test_planted_random_layout():
    chains, offsets, ids, p, starts, lengths = planted_random()
    arcs, arc_off, classes, reads = planted_reference("random")
    inside = [any(j != i and starts[j] <= starts[i] and starts[i] + lengths[i] <= starts[j] + lengths[j] and
                  (lengths[j] > lengths[i] or (lengths[j] == lengths[i] and ids[j] < ids[i])) for j in range(120)) for i in range(120)]
    flagged = np.zeros(120, bool)
    flagged[ids] = inside
    assert ((reads["flags"] & A.SG_READ_CONTAINED) != 0).tolist() == flagged.tolist() and 10 < flagged.sum() < 110
    assert out_degrees(reads).max() == 1 and len(arcs) > 2 * int((arcs["flags"] == 0).sum()) > 0
    assert reduced_records(arcs) == reference_myers(arc_tuples(arcs), p["fuzz"])


@pytest.mark.parametrize("n", [63, 64, 65, 66, 130])
def test_planted_piles(n):
    chains, offsets, ids, p = planted_pile(n)
    arcs, arc_off, classes, reads = planted_reference("pile", n)
    assert len(arcs) == n * (n - 1) and int((arcs["flags"] == 0).sum()) == 2 * (n - 1)
    assert int((arc_off[1:] - arc_off[:-1]).max()) == n - 1
    assert reduced_records(arcs) == reference_myers(arc_tuples(arcs), p["fuzz"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hostile_graphs_contain_myers(seed):
    rng = np.random.default_rng(seed)
    lengths = rng.integers(300, 700, 60)
    starts = np.array([rng.integers(0, 2500) for _ in lengths])
    chains, offsets, _ = layout_records(starts, lengths, seed=seed, perturb=60, doubled=0.1)
    arcs = reference_graph(chains, None, offsets, **params(fuzz=20))[0]
    assert len(arcs) > 50 and len(set(arc_tuples(arcs))) == len(arcs)  # (enough arcs for the comparison to mean something)
    assert len(set(x[:2] for x in arc_tuples(arcs))) < len(arcs)  # doubled records: duplicate arcs are there
    assert reduced_records(arcs) >= reference_myers(arc_tuples(arcs), 20)


# ---- what the library refuses before it launches anything: no device needed ----------------------------------------------------
def test_bad_arguments_need_no_device():
    """a context cannot be made without a device, so only the first refusal of both entry points, the null context, runs here; the
    others (flags, permille bounds, mem, 2^31) are in tests/test_gpu_string_graph.py"""
    from kmerutils_amd import build, lib
    build.build()
    L = lib.load()
    chains, off = records([(0, 1, 0, 600, 1000, 0, 400)]), offsets_of([1000, 1000])
    cls, reads, arcs, arc_off = np.zeros(1, np.uint8), np.zeros(2, READ), np.zeros(2, ARC), np.zeros(5, np.uint64)
    total, p = C.c_uint64(7), A.SgParams(50, 1000, 250, 0, 0, 0)
    assert C.sizeof(A.SgParams) == 24 and C.sizeof(A.SgRead) == READ.itemsize == 16 and C.sizeof(A.SgArc) == ARC.itemsize == 32
    assert L.kmu_sg_classify(None, chains.ctypes.data, None, 1, off.ctypes.data, 2, C.byref(p), A.MEM_HOST, cls.ctypes.data,
                             reads.ctypes.data) == A.E_BAD_ARG
    assert L.kmu_sg_graph(None, chains.ctypes.data, None, 1, off.ctypes.data, 2, C.byref(p), A.MEM_HOST, cls.ctypes.data, reads.ctypes.data,
                          arcs.ctypes.data, 2, arc_off.ctypes.data, C.byref(total)) == A.E_BAD_ARG
    assert b"null" in L.kmu_last_error(None)
    assert total.value == 7 and not cls.any() and not arcs.view(np.uint32).any() and not reads.view(np.uint32).any()

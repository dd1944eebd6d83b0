"""-m "not gpu": string graph cleaning without a device.  reference_clean, sequential walks written from the contract of
kmu_sg_clean in include/kmu.h, which the device tests compare against; `planted`, backbones with dead ends and alternative paths
whose removal is known; the layouts of the string graph tests, from which nothing may be removed; and the refusals the library makes
before it needs a context."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import ARC, READ, Refused, offsets_of, planted_reference  # noqa: E402
from test_unitigs_abi import arcs_of, hostile_graph, reference_unitigs, with_mates  # noqa: E402

STATS = A.SG_CLEAN_STATS
LIMITS = [(4, 8), (1, 1), (0, 8), (4, 0), (64, 64)]


def reference_clean(arcs, n_reads, T, B, reads=None):
    """(arcs_out, reads_out, stats) of the contract: the faults, then tips, then bubbles, then unique and the degrees"""
    arcs = np.asarray(arcs)
    rows, n_v = arcs.tolist(), 2 * n_reads
    for i in range(1, len(rows)):
        if rows[i][0] < rows[i - 1][0]:
            raise Refused("from decreases at arc %d" % i)
    alive = [r[5] == 0 for r in rows]
    keys = set()
    for i, (v, w, _, _, c, _, _, _) in enumerate(rows):
        if not alive[i]:
            continue
        if v >= n_v or w >= n_v or v >> 1 == w >> 1:
            raise Refused("arc %d -> %d" % (v, w))
        if reads is not None and (int(reads["flags"][v >> 1]) | int(reads["flags"][w >> 1])) & A.SG_READ_CONTAINED:
            raise Refused("arc %d -> %d touches a contained read" % (v, w))
        keys.add((v, w, c))
    for v, w, c in keys:
        if (w ^ 1, v ^ 1, c) not in keys:
            raise Refused("no mate for %d -> %d" % (v, w))
    new_arc, new_read = [0] * len(rows), [0] * n_reads
    stats = dict.fromkeys(STATS, 0)

    def out_lists():
        out = {}
        for i, r in enumerate(rows):
            if alive[i]:
                out.setdefault(r[0], []).append(r[1])
        return out

    def remove(removed, arc_bit, read_bit, count):
        for r in removed:
            new_read[r] |= read_bit
        for i, r in enumerate(rows):
            if alive[i] and (r[0] >> 1 in removed or r[1] >> 1 in removed):
                alive[i], new_arc[i] = False, arc_bit
                stats[count] += 1

    if T:
        out = out_lists()
        deg = lambda v: len(out.get(v, ()))  # noqa: E731
        ends = {}  # the last vertex of a candidate tip: its reads, in walk order
        for v0 in range(n_v):
            if deg(v0 ^ 1) != 0 or deg(v0) != 1:
                continue
            walk = [v0]
            while True:
                w = out[walk[-1]][0]
                if deg(w ^ 1) >= 2:
                    if len(walk) <= T:
                        ends[walk[-1]] = walk
                    break
                if deg(w) == 1 and len(walk) < T:
                    walk.append(w)
                else:
                    break
        spared = set()
        for w in range(n_v):
            if deg(w ^ 1) < 2:
                continue
            before = [x ^ 1 for x in out[w ^ 1]]
            if all(u in ends for u in before):
                spared.add(min(before, key=lambda u: (-len(ends[u]), u)))
                stats["n_spared"] += 1
        removed = set()
        for u, walk in ends.items():
            if u not in spared:
                stats["n_tips"] += 1
                stats["n_tip_reads"] += len(walk)
                removed.update(v >> 1 for v in walk)
        remove(removed, A.SG_ARC_TIP, A.SG_READ_TIP, "n_arcs_tip")
    if B:
        out = out_lists()
        deg = lambda v: len(out.get(v, ()))  # noqa: E731

        def branch(a1):
            inner, x = [], a1
            while len(inner) < B:
                if deg(x ^ 1) != 1 or deg(x) != 1:
                    return None
                inner.append(x)
                x = out[x][0]
                if deg(x ^ 1) == 2:
                    return inner, x
            return None
        removed = set()
        for s in range(n_v):
            if deg(s) != 2:
                continue
            one, two = branch(out[s][0]), branch(out[s][1])
            if one is None or two is None or one[1] != two[1] or one[1] >> 1 == s >> 1:
                continue
            t = one[1]
            a, b = [v >> 1 for v in one[0]], [v >> 1 for v in two[0]]
            assert not set(a) & set(b)  # the proof of the header
            if len(a) != len(b):
                loser = a if len(a) < len(b) else b
            else:
                loser = b if min(a) < min(b) else a
            removed.update(loser)
            if s < t ^ 1:
                stats["n_bubbles"] += 1
                stats["n_bubble_reads"] += len(loser)
        remove(removed, A.SG_ARC_BUBBLE, A.SG_READ_BUBBLE, "n_arcs_bubble")
    out = out_lists()
    arcs_out = arcs.copy()
    reads_out = np.zeros(n_reads, READ) if reads is None else np.array(reads, copy=True)
    for i, (v, w, _, _, _, flags, _, _) in enumerate(rows):
        arcs_out["flags"][i] = flags | new_arc[i]
        arcs_out["unique"][i] = int(alive[i] and len(out[v]) == 1 and len(out[w ^ 1]) == 1)
    stats["n_arcs_left"] = sum(alive)
    for r in range(n_reads):
        reads_out[r] = (int(reads_out["flags"][r]) | new_read[r], int(reads_out["n_records"][r]), len(out.get(2 * r, ())),
                        len(out.get(2 * r + 1, ())))
    return arcs_out, reads_out, stats


# ---- planted graphs --------------------------------------------------------------------------------------------------------------
def planted(n_back, tips, bubbles, seed, copies=1):
    """`copies` disjoint backbones of n_back reads, each with the same plants, ids and strands shuffled over all of them.
    bubbles: (k, m, pos) -- k reads from backbone[pos] to backbone[pos + m + 1], around m backbone reads.
    tips: (n, where, leaves) -- a chain of n reads that enters `where` (leaves it if `leaves`); where is a backbone position, or
    (j, i): read i of bubble j's alternative.
    Returns (arcs, n_reads, groups): arcs with their mates, sorted; groups[c] = dict(backbone, bypassed, alts, tips) of read ids."""
    rng = np.random.default_rng(seed)
    edges, n_nodes = [(i, i + 1) for i in range(n_back - 1)], n_back
    alts, bypassed, chains = [], [], []
    for k, m, pos in bubbles:
        alt = list(range(n_nodes, n_nodes + k))
        n_nodes += k
        edges += list(zip([pos] + alt, alt + [pos + m + 1]))
        alts.append(alt)
        bypassed.append(list(range(pos + 1, pos + m + 1)))
    for n, where, leaves in tips:
        chain = list(range(n_nodes, n_nodes + n))
        n_nodes += n
        at = where if isinstance(where, int) else alts[where[0]][where[1]]
        edges += list(zip([at] + chain, chain)) if leaves else list(zip(chain, chain[1:] + [at]))
        chains.append(chain)
    n_reads = n_nodes * copies
    ids, flip, lens = rng.permutation(n_reads), rng.integers(0, 2, n_reads), rng.integers(500, 600, n_reads)
    rows, groups = [], []
    for c in range(copies):
        base = c * n_nodes
        vertex = lambda x: 2 * int(ids[base + x]) + int(flip[base + x])  # noqa: E731
        rows += [(vertex(a), vertex(b), int(rng.integers(150, 250))) for a, b in edges]
        read = lambda xs: [int(ids[base + x]) for x in xs]  # noqa: E731
        groups.append(dict(backbone=read(range(n_back)), bypassed=[read(x) for x in bypassed], alts=[read(x) for x in alts],
                           tips=[read(x) for x in chains]))
    by_id = np.zeros(n_reads, np.int64)
    by_id[ids] = lens
    arcs = arcs_of(with_mates(rows, by_id), unique=0)
    return arcs[np.lexsort((arcs["rec"], arcs["to"], arcs["from"]))], n_reads, groups


BUBBLES7 = [(1, 1, 2), (2, 1, 6), (1, 2, 10), (3, 3, 15), (8, 2, 22), (9, 2, 28), (2, 8, 34)]
MIX = dict(n_back=65,
           tips=[(n, 4 + 4 * n, False) for n in range(1, 6)] + [(1, 28, True), (2, 31, True), (3, 34, True), (2, 0, False), (3, 0, False)],
           bubbles=[(1, 1, 37), (2, 1, 41), (3, 3, 45), (8, 2, 51), (2, 2, 56)])
CASES = {
    "tips in": dict(n_back=40, tips=[(n, 5 * n, False) for n in range(1, 6)], bubbles=[]),
    "tips out": dict(n_back=40, tips=[(n, 5 * n, True) for n in range(1, 6)], bubbles=[]),
    "two into the first": dict(n_back=20, tips=[(2, 0, False), (3, 0, False)], bubbles=[]),
    "two out of the last": dict(n_back=20, tips=[(2, 19, True), (2, 19, True)], bubbles=[]),
    "bubbles": dict(n_back=60, tips=[], bubbles=BUBBLES7),
    "three adjacent": dict(n_back=20, tips=[], bubbles=[(2, 1, 5), (1, 1, 7), (3, 2, 9)]),
    "tip on a branch": dict(n_back=20, tips=[(1, (0, 1), False)], bubbles=[(3, 1, 5)]),
    "mix": MIX,
}
# what (T, B) = (4, 8) removes: n_tips, n_tip_reads, n_spared, n_bubbles, n_bubble_reads
AT_4_8 = {"tips in": (4, 10, 0, 0, 0), "tips out": (4, 10, 0, 0, 0), "two into the first": (1, 2, 1, 0, 0),
          "two out of the last": (1, 2, 1, 0, 0), "bubbles": (0, 0, 0, 6, 10), "three adjacent": (0, 0, 0, 3, 4),
          "tip on a branch": (1, 1, 0, 1, 1), "mix": (8, 18, 1, 5, 9)}


@functools.lru_cache(maxsize=None)
def planted_case(name, seed=1, copies=1):
    """(arcs, n_reads, groups) of a case, built once (device tests included)"""
    return planted(seed=seed, copies=copies, **CASES[name])


@functools.lru_cache(maxsize=None)
def cleaned_case(name, T, B, seed=1, copies=1):
    arcs, n_reads, _ = planted_case(name, seed, copies)
    return reference_clean(arcs, n_reads, T, B)


def removed_reads(reads):
    return set(np.flatnonzero(reads["flags"] & (A.SG_READ_TIP | A.SG_READ_BUBBLE)).tolist())


def mate_symmetric(arcs):
    left = arcs[arcs["flags"] == 0]
    keys = set(zip(left["from"].tolist(), left["to"].tolist(), left["rec"].tolist()))
    return all((w ^ 1, v ^ 1, c) in keys for v, w, c in keys)


@pytest.mark.parametrize("T,B", LIMITS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_cases(name, T, B):
    arcs, n_reads, groups = planted_case(name)
    arcs_out, reads_out, stats = cleaned_case(name, T, B)
    g = groups[0]
    planted_ids = set(sum(g["bypassed"] + g["alts"] + g["tips"], []))
    gone = removed_reads(reads_out)
    # a backbone read goes only where an alternative around it was planted
    assert gone <= planted_ids
    assert len(gone) == stats["n_tip_reads"] + stats["n_bubble_reads"]
    assert mate_symmetric(arcs_out) and stats["n_arcs_left"] == int((arcs_out["flags"] == 0).sum())
    assert stats["n_arcs_tip"] + stats["n_arcs_bubble"] + stats["n_arcs_left"] == len(arcs)
    assert (T or not stats["n_tips"]) and (B or not stats["n_bubbles"])
    # every surviving arc joins two reads that are left; the layout accepts the result
    left = arcs_out[arcs_out["flags"] == 0]
    assert not gone & set((left["from"] >> 1).tolist()) and not gone & set((left["to"] >> 1).tolist())
    unitigs, path, place = reference_unitigs(arcs_out, minimizer.layout_reads(reads_out), offsets_of(np.full(n_reads, 1000)))
    assert (place["unitig"][np.array(sorted(gone), np.int64)] == A.SG_NONE).all() and len(path) == n_reads - len(gone)
    if (T, B) == (4, 8):
        assert tuple(stats[k] for k in STATS[:5]) == AT_4_8[name]
    # the output is a valid input: a second round keeps every flag of the first
    again = reference_clean(arcs_out, n_reads, T, B, reads_out)
    assert ((again[0]["flags"] & arcs_out["flags"]) == arcs_out["flags"]).all()


def test_what_goes_at_4_8():
    """the planted reads by name: which tips go, which branch of every bubble"""
    g = planted_case("tips in")[2][0]
    gone = removed_reads(cleaned_case("tips in", 4, 8)[1])
    assert gone == set(sum(g["tips"][:4], [])) and not gone & set(g["tips"][4])  # the tip of 5 reads stays
    g = planted_case("tips out")[2][0]
    assert removed_reads(cleaned_case("tips out", 4, 8)[1]) == set(sum(g["tips"][:4], []))
    g = planted_case("two into the first")[2][0]
    assert removed_reads(cleaned_case("two into the first", 4, 8)[1]) == set(g["tips"][0])  # the tip of 3 is spared
    g = planted_case("two out of the last")[2][0]
    gone = removed_reads(cleaned_case("two out of the last", 4, 8)[1])
    assert gone in (set(g["tips"][0]), set(g["tips"][1]))
    g = planted_case("bubbles")[2][0]
    gone = removed_reads(cleaned_case("bubbles", 4, 8)[1])
    want = set()
    for (k, m, _), alt, by in zip(BUBBLES7, g["alts"], g["bypassed"]):
        if k > 8:
            continue  # the branch of 9 reads is no branch: both stay
        want.update((alt if k < m else by) if k != m else (by if min(alt) < min(by) else alt))
    assert gone == want and not gone & set(g["alts"][5]) and not gone & set(g["bypassed"][5])
    g = planted_case("tip on a branch")[2][0]
    arcs_out, reads_out, _ = cleaned_case("tip on a branch", 4, 8)
    assert set(np.flatnonzero(reads_out["flags"] & A.SG_READ_TIP).tolist()) == set(g["tips"][0])
    assert set(np.flatnonzero(reads_out["flags"] & A.SG_READ_BUBBLE).tolist()) == set(g["bypassed"][0])
    assert not removed_reads(cleaned_case("tip on a branch", 0, 8)[1])  # with the tip in place the branch is no branch


def test_the_tie_of_two_tips_spares_the_smaller_last_vertex():
    arcs, n_reads, groups = planted_case("two out of the last")
    arcs_out, reads_out, stats = cleaned_case("two out of the last", 4, 8)
    last = groups[0]["backbone"][-1]
    # the tips leave the last backbone read on the strand it was given; their twins enter its other vertex
    v = [int(x["from"]) for x in arcs if int(x["from"]) >> 1 == last and int(x["to"]) >> 1 in sum(groups[0]["tips"], [])][0]
    ends = sorted(int(x["to"]) ^ 1 for x in arcs if int(x["from"]) == v)
    assert len(ends) == 2 and not int(reads_out["flags"][ends[0] >> 1]) and int(reads_out["flags"][ends[1] >> 1]) == A.SG_READ_TIP


@pytest.mark.parametrize("n,T,gone", [(63, 64, 63), (64, 64, 64), (65, 64, 0), (3, 3, 3), (4, 3, 0)])
def test_tip_walk_limits(n, T, gone):
    arcs, n_reads, groups = planted(n + 70, [(n, n + 2, False)], [], seed=n)
    assert len(removed_reads(reference_clean(arcs, n_reads, T, 0)[1])) == gone


@pytest.mark.parametrize("k,B,gone", [(64, 64, 2), (65, 64, 0), (2, 2, 1), (3, 2, 0)])
def test_branch_walk_limits(k, B, gone):
    """a branch of k reads around one of 1 or 2 backbone reads: popped iff k <= B, and then the shorter backbone stretch goes"""
    arcs, n_reads, groups = planted(12, [], [(k, gone or 1, 4)], seed=k)
    assert removed_reads(reference_clean(arcs, n_reads, 0, B)[1]) == (set(groups[0]["bypassed"][0]) if gone else set())


# ---- nothing to remove -----------------------------------------------------------------------------------------------------------
def nothing_removed(arcs, reads, n_reads):
    for T, B in LIMITS:
        arcs_out, reads_out, stats = reference_clean(arcs, n_reads, T, B, reads)
        assert arcs_out.tobytes() == arcs.tobytes() and reads_out.tobytes() == reads.tobytes()
        assert [stats[k] for k in STATS[:7]] == [0] * 7 and stats["n_arcs_left"] == int((arcs["flags"] == 0).sum())


@pytest.mark.parametrize("name,arg", [("tiling", 0), ("tiling", 3), ("random", None), ("pile", 65)])
def test_planted_layouts_come_back_as_they_are(name, arg):
    arcs, _, _, reads = planted_reference(name, arg)
    nothing_removed(arcs, reads, len(reads))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hostile_graphs_come_back_as_they_are(seed):
    arcs, reads, _, _ = hostile_graph(seed)
    nothing_removed(arcs, reads, len(reads))


# ---- faults ----------------------------------------------------------------------------------------------------------------------
def faulty_graphs():
    """name -> (arcs, reads or None, n_reads): one planted fault each, on a line of four reads"""
    lens = [1000] * 4
    good = arcs_of(with_mates([(0, 2, 600), (2, 4, 600), (4, 6, 600)], lens), unique=0)
    good = good[np.lexsort((good["rec"], good["to"], good["from"]))]
    out = {}

    def edit(name, fn, reads=None):
        x = good.copy()
        x = fn(x) if fn else x
        out[name] = (x, reads, 4)
    edit("unsorted", lambda x: x[[1, 0, 2, 3, 4, 5]])

    def beyond(x):
        x["to"][-1] = 8  # (the last arc: `from` stays sorted)
        return x
    edit("out of range", beyond)

    def within(x):
        x["to"][-1] = int(x["from"][-1]) ^ 1
        return x
    edit("within one read", within)
    edit("no mate", lambda x: x[:-1])

    def other_rec(x):
        x["rec"][-1] = 7
        return x
    edit("mate of another rec", other_rec)
    reads = np.zeros(4, READ)
    reads["flags"][1] = A.SG_READ_CONTAINED
    edit("contained", None, reads)
    return out


def test_every_fault_is_refused():
    for name, (arcs, reads, n_reads) in faulty_graphs().items():
        with pytest.raises(Refused):
            reference_clean(arcs, n_reads, 4, 8, reads)
        # the same fault in an arc that does not survive counts for nothing, except the order of `from`
        if name not in ("unsorted", "contained", "no mate"):
            dead = arcs.copy()
            dead["flags"][-1] = A.SG_ARC_REDUCED
            mate = np.flatnonzero((dead["rec"] == 2) & (dead["flags"] == 0))
            dead["flags"][mate] = A.SG_ARC_REDUCED
            reference_clean(dead, n_reads, 4, 8, None)


# ---- what the library refuses before it needs a context: no device needed ----------------------------------------------------------
def test_bad_arguments_need_no_device():
    from kmerutils_amd import build, lib
    build.build()
    L = lib.load()
    assert C.sizeof(A.SgCleanParams) == 16 and C.sizeof(A.SgCleanStats) == np.dtype(A.SG_CLEAN_STATS_DTYPE).itemsize == 64
    arcs, n_reads, _ = planted_case("tips in")
    arcs_out, reads_out = np.zeros(len(arcs), ARC), np.zeros(n_reads, READ)
    stats = A.SgCleanStats(*([7] * 8))

    def call(p=(4, 8, 0, 0), a=arcs.ctypes.data, n=len(arcs), r=n_reads, mem=A.MEM_HOST, out=arcs_out.ctypes.data, st=C.byref(stats), ctx=None,
             no_p=False):
        return L.kmu_sg_clean(ctx, a, n, None, r, None if no_p else C.byref(A.SgCleanParams(*p)), mem, out, reads_out.ctypes.data, st)
    bad = [(dict(no_p=True), b"null"), (dict(st=None), b"null"), (dict(a=None), b"null"), (dict(out=None), b"null"),
           (dict(p=(4, 8, 1, 0)), b"flags"), (dict(p=(4, 8, 0, 1)), b"zero"), (dict(p=(65, 8, 0, 0)), b"at most 64"),
           (dict(p=(4, 65, 0, 0)), b"at most 64"), (dict(mem=7), b"bad mem"), (dict(r=0), b"no reads"),
           (dict(out=arcs.ctypes.data), b"overlaps"), (dict(out=arcs.ctypes.data + 32 * (len(arcs) - 1)), b"overlaps"), (dict(), b"null context")]
    for kw, word in bad:
        assert call(**kw) == A.E_BAD_ARG and word in L.kmu_last_error(None), (kw, L.kmu_last_error(None))
    assert call(r=1 << 31) == A.E_UNSUPPORTED and b"2^31" in L.kmu_last_error(None)
    assert call(n=1 << 32) == A.E_UNSUPPORTED and b"2^32" in L.kmu_last_error(None)
    assert [getattr(stats, k) for k in STATS] == [7] * 8 and not arcs_out.view(np.uint32).any() and not reads_out.view(np.uint32).any()


def test_wrappers_on_the_host():
    """layout_reads and gfa_lines need no device"""
    arcs, n_reads, groups = planted_case("tips in")
    arcs_out, reads_out, _ = cleaned_case("tips in", 4, 8)
    laid = minimizer.layout_reads(reads_out)
    gone = sorted(removed_reads(reads_out))
    assert (laid["flags"][gone] == A.SG_READ_TIP | A.SG_READ_CONTAINED).all() and int((laid["flags"] != 0).sum()) == len(gone)
    assert reads_out["flags"].max() == A.SG_READ_TIP  # a copy
    names, off = ["r%d" % r for r in range(n_reads)], offsets_of(np.full(n_reads, 1000))
    before, after = minimizer.gfa_lines(arcs, names, off), minimizer.gfa_lines(arcs_out, names, off, reads=reads_out)
    assert len(before) == n_reads + len(arcs) and len(after) == n_reads - len(gone) + int((arcs_out["flags"] == 0).sum())
    assert set(after) <= set(before) and not any("r%d" % gone[0] in line.split("\t") for line in after)

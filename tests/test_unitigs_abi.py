"""-m "not gpu": the unitig layout without a device.  reference_unitigs and reference_sequences, sequential walks written from the
contract in include/kmu.h, which the device tests compare against; the planted layouts and the hand cases that make them
trustworthy; and the refusal both entry points make before they launch anything."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import (ARC, READ, Refused, layout_records, offsets_of, params, planted_pile, planted_random,  # noqa: E402
                                   planted_reference, planted_tiling, reference_graph)

STEP, UNITIG, PLACE = np.dtype(A.SG_STEP_DTYPE), np.dtype(A.SG_UNITIG_DTYPE), np.dtype(A.SG_PLACE_DTYPE)
NONE = A.SG_NONE


def arcs_of(rows, unique=1, flags=0):
    """arc records from (from, to, len) rows: unique arcs that are not reduced unless said otherwise"""
    out = np.zeros(len(rows), ARC)
    for i, (v, w, ln) in enumerate(rows):
        out[i] = (v, w, ln, 0, i // 2, flags, unique, 0)
    return out


def with_mates(rows, lens):
    """the arcs v -> w of `rows` and their mates w^1 -> v^1, each as long as the overhang it leaves on reads of the lengths `lens`
    (an arc v -> w of length l between reads of la and lb bases has a mate of length la - (lb - l))"""
    out = []
    for v, w, ln in rows:
        out += [(v, w, ln), (w ^ 1, v ^ 1, int(lens[v >> 1]) - (int(lens[w >> 1]) - ln))]
    return out


def reference_unitigs(arcs, reads, offsets):
    """(unitigs, path, place) of the contract, by walking"""
    off = [int(x) for x in offsets]
    n_reads = len(off) - 1
    n_v = 2 * n_reads
    length = [off[r + 1] - off[r] for r in range(n_reads)]
    contained = [reads is not None and bool(int(reads["flags"][r]) & A.SG_READ_CONTAINED) for r in range(n_reads)]
    nxt, prv, inn = {}, {}, {}
    for v, w, ln, _, _, flags, unique, _ in np.asarray(arcs).tolist():
        if unique != 1:
            continue
        if v >= n_v or w >= n_v or v >> 1 == w >> 1 or ln > length[w >> 1] or flags & A.SG_ARC_REDUCED:
            raise Refused("arc %d -> %d" % (v, w))
        if contained[v >> 1] or contained[w >> 1] or v in nxt or w in prv:
            raise Refused("arc %d -> %d" % (v, w))
        nxt[v], prv[w], inn[w] = w, v, ln
    for v, w in nxt.items():
        if nxt.get(w ^ 1) != v ^ 1:
            raise Refused("no mate for %d -> %d" % (v, w))
    found, seen = [], set()
    for v in range(n_v):  # the paths, from their vertex without prev
        if v in prv or contained[v >> 1]:
            continue
        walk = [v]
        while walk[-1] in nxt:
            walk.append(nxt[walk[-1]])
        seen.update(walk)
        found.append((walk, 0))
    for v in range(n_v):  # what is left lies on cycles; ascending v meets the smallest vertex of each first
        if v in seen or contained[v >> 1]:
            continue
        walk = [v]
        while nxt[walk[-1]] != v:
            walk.append(nxt[walk[-1]])
        seen.update(walk)
        found.append((walk, A.SG_UNITIG_CIRCULAR))
    kept = sorted((min(walk) >> 1, walk, flags) for walk, flags in found if min(walk) % 2 == 0)
    unitigs, path, place = np.zeros(len(kept), UNITIG), [], np.zeros(n_reads, PLACE)
    place["unitig"][contained] = NONE
    for u, (min_read, walk, flags) in enumerate(kept):
        first, end = len(path), 0
        for rank, v in enumerate(walk):
            end += inn[v] if v in inn else length[v >> 1]
            path.append((v >> 1, v & 1, end))
            place[v >> 1] = (u, rank, v & 1, 0)
        unitigs[u] = (first, end, len(walk), flags, min_read, 0)
    return unitigs, np.array(path, STEP) if path else np.zeros(0, STEP), place


_COMPLEMENT = np.full(256, ord("N"), np.uint8)
for _a, _b in ("AT", "CG", "at", "cg"):
    _COMPLEMENT[ord(_a)], _COMPLEMENT[ord(_b)] = ord(_b), ord(_a)


def reference_sequences(unitigs, path, bases, offsets):
    """(seq, seq_offsets) of the contract, a byte loop per step"""
    off = [int(x) for x in offsets]
    n_reads, n_steps = len(off) - 1, len(path)
    bases = np.asarray(bases, np.uint8)
    seqs = []
    for first, length, n, _, _, _ in np.asarray(unitigs).tolist():
        if first + n > n_steps:
            raise Refused("steps %d + %d of %d" % (first, n, n_steps))
        parts, before = [], 0
        for read, strand, end in np.asarray(path)[first:first + n].tolist():
            if read >= n_reads or strand > 1 or end < before or end - before > off[read + 1] - off[read]:
                raise Refused("step (%d, %d, %d)" % (read, strand, end))
            c, whole = end - before, bases[off[read]:off[read + 1]]
            oriented = _COMPLEMENT[whole[::-1]] if strand else whole
            parts.append(oriented[len(oriented) - c:])
            before = end
        if before != length:
            raise Refused("the last end %d is not len %d" % (before, length))
        seqs.append(np.concatenate(parts) if parts else np.zeros(0, np.uint8))
    seq_off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    return (np.concatenate(seqs) if seqs else np.zeros(0, np.uint8)).astype(np.uint8), seq_off


def steps_of(unitigs, path, u):
    x = unitigs[u]
    return [tuple(int(v) for v in s) for s in path[int(x["first"]):int(x["first"]) + int(x["n_reads"])].tolist()]


@functools.lru_cache(maxsize=None)
def planted_unitigs(name, arg=None):
    """(arcs, reads, offsets, ids) of a planted layout and its reference_unitigs, computed once (device tests included)"""
    case = {"tiling": planted_tiling, "random": planted_random, "pile": planted_pile}[name]
    got = case(arg) if arg is not None else case()
    arcs, _, _, reads = planted_reference(name, arg)
    return (arcs, reads, got[1], got[2]), reference_unitigs(arcs, reads, got[1])


@functools.lru_cache(maxsize=None)
def hostile_graph(seed):
    """the graph of test_hostile_graphs_contain_myers at fuzz 20"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(300, 700, 60)
    starts = np.array([rng.integers(0, 2500) for _ in lengths])
    chains, offsets, _ = layout_records(starts, lengths, seed=seed, perturb=60, doubled=0.1)
    arcs, _, _, reads = reference_graph(chains, None, offsets, **params(fuzz=20))
    return arcs, reads, offsets, chains


def circle_arcs(n, lens, arc_len, seed):
    """a circle of n reads with shuffled ids and strands as arcs with their mates: read i of the circle continues into read i + 1
    by arc_len[i + 1] bases.  Returns (arcs, offsets, vertices): the circle's vertices in walk order"""
    rng = np.random.default_rng(seed)
    ids, flip = rng.permutation(n), rng.integers(0, 2, n)
    vs = [2 * int(ids[i]) + int(flip[i]) for i in range(n)]
    by_id = np.zeros(n, np.int64)
    by_id[ids] = lens
    rows = with_mates([(vs[i], vs[(i + 1) % n], int(arc_len[(i + 1) % n])) for i in range(n)], by_id)
    return arcs_of(rows), offsets_of(by_id), vs


# ---- planted layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 3])
def test_planted_tiling(jitter):
    (arcs, reads, offsets, ids), (unitigs, path, place) = planted_unitigs("tiling", jitter)
    assert len(unitigs) == 1 and len(path) == 27 and int(unitigs["n_reads"][0]) == 27 and not unitigs["flags"][0]
    order = path["read"].tolist()
    assert order in ([int(r) for r in ids], [int(r) for r in ids[::-1]])  # line order, or its reverse
    assert int(unitigs["min_read"][0]) == 0 and int(path["strand"][order.index(0)]) == 0
    assert place["unitig"].tolist() == [0] * 27 and sorted(place["rank"].tolist()) == list(range(27))
    assert int(unitigs["len"][0]) == (3000 if jitter == 0 else int(path["end"][-1]))
    if jitter == 0:
        assert path["end"].tolist() == [400 + 100 * i for i in range(27)]
    else:
        assert abs(int(unitigs["len"][0]) - 3000) <= 27 * 6 and (np.diff(path["end"].astype(np.int64)) > 0).all()


def test_planted_random_layout():
    (arcs, reads, offsets, ids), (unitigs, path, place) = planted_unitigs("random")
    contained = (reads["flags"] & A.SG_READ_CONTAINED) != 0
    assert len(unitigs) == 1 and len(path) == 37 and int(contained.sum()) == 83 and int(unitigs["len"][0]) == 3982
    assert (place["unitig"][contained] == NONE).all() and not place["rank"][contained].any() and not place["strand"][contained].any()
    assert (place["unitig"][~contained] == 0).all() and sorted(path["read"].tolist()) == np.flatnonzero(~contained).tolist()


def test_planted_pile():
    (arcs, reads, offsets, ids), (unitigs, path, place) = planted_unitigs("pile", 65)
    assert len(unitigs) == 1 and len(path) == 65 and int(unitigs["len"][0]) == 528 and not (reads["flags"] & A.SG_READ_CONTAINED).any()
    assert path["end"].tolist() == [400 + 2 * i for i in range(65)]


@pytest.mark.parametrize("seed,sizes", [(1, [2, 3, 11]), (2, [2, 6, 10]), (3, [4, 6, 11])])
def test_hostile_graphs(seed, sizes):
    arcs, reads, offsets, _ = hostile_graph(seed)
    unitigs, path, place = reference_unitigs(arcs, reads, offsets)
    contained = (reads["flags"] & A.SG_READ_CONTAINED) != 0
    linked = np.zeros(60, bool)
    for x in arcs[arcs["unique"] == 1]:
        linked[int(x["from"]) >> 1] = linked[int(x["to"]) >> 1] = True
    assert not (linked & contained).any()
    assert sorted(unitigs["n_reads"][unitigs["n_reads"] > 1].tolist()) == sizes
    assert int((unitigs["n_reads"] == 1).sum()) == int((~contained & ~linked).sum())
    assert len(path) == int((~contained).sum()) and not unitigs["flags"].any()


# ---- hand cases ----------------------------------------------------------------------------------------------------------------
def test_the_smoke_line_of_three_reads():
    """three reads of 1 000 bases, each 100 to the right of the one before (the line of smoke())"""
    off = offsets_of([1000, 1000, 1000])
    arcs = arcs_of(with_mates([(0, 2, 100), (2, 4, 100)], [1000] * 3))
    unitigs, path, place = reference_unitigs(arcs, None, off)
    assert unitigs.tolist() == [(0, 1200, 3, 0, 0, 0)]
    assert path.tolist() == [(0, 0, 1000), (1, 0, 1100), (2, 0, 1200)]
    assert place.tolist() == [(0, 0, 0, 0), (0, 1, 0, 0), (0, 2, 0, 0)]
    # no arcs at all: every read is its own unitig
    unitigs, path, place = reference_unitigs(np.zeros(0, ARC), None, off)
    assert unitigs.tolist() == [(r, 1000, 1, 0, r, 0) for r in range(3)] and path.tolist() == [(r, 0, 1000) for r in range(3)]


@pytest.mark.parametrize("sa,sb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_the_four_strand_combinations(sa, sb):
    """one arc from read 0 on strand sa into read 1 on strand sb, 300 bases long; reads of 1 000 and 800"""
    off = offsets_of([1000, 800])
    arcs = arcs_of(with_mates([(sa, 2 + sb, 300)], [1000, 800]))
    unitigs, path, place = reference_unitigs(arcs, None, off)
    if sa == 0:  # read 0 forward is walked first
        assert path.tolist() == [(0, 0, 1000), (1, sb, 1300)]
    else:  # the twin is kept: read 1 on the other strand leads into read 0 forward by 1000 - (800 - 300)
        assert path.tolist() == [(1, sb ^ 1, 800), (0, 0, 1300)]
    assert unitigs.tolist() == [(0, 1300, 2, 0, 0, 0)]


def test_orientation_rule():
    """read 1 forward runs into read 0 reversed: the smallest read is reversed in walk order, so the twin is kept"""
    off = offsets_of([500, 700])
    arcs = arcs_of(with_mates([(2, 1, 200)], [500, 700]))
    unitigs, path, place = reference_unitigs(arcs, None, off)
    assert path.tolist() == [(0, 0, 500), (1, 1, 900)] and unitigs.tolist() == [(0, 900, 2, 0, 0, 0)]
    assert place.tolist() == [(0, 0, 0, 0), (0, 1, 1, 0)]


@pytest.mark.parametrize("n", [3, 4, 64, 65])
def test_circles(n):
    rng = np.random.default_rng(n)
    lens, arc_len = rng.integers(500, 600, n), rng.integers(150, 250, n)  # (every mate's length stays inside its read)
    arcs, off, vs = circle_arcs(n, lens, arc_len, seed=n)
    unitigs, path, place = reference_unitigs(arcs, None, off)
    assert len(unitigs) == 1 and len(path) == n
    u = unitigs[0]
    assert int(u["flags"]) == A.SG_UNITIG_CIRCULAR and int(u["min_read"]) == 0 and int(u["n_reads"]) == n
    assert (int(path["read"][0]), int(path["strand"][0])) == (0, 0)  # the start is vertex 2 * min_read
    # the circumference: on the strand as built, the sum of its arcs; on the twin strand, the sum of the mates
    at = vs.index(0) if 0 in vs else None
    if at is not None:
        assert int(u["len"]) == int(arc_len.sum())
        assert path["read"].tolist() == [vs[(at + i) % n] >> 1 for i in range(n)]
    else:
        mates = arcs[1::2]
        assert int(u["len"]) == int(mates["len"].sum())


def test_every_arc_fault_is_refused():
    off, lens = offsets_of([1000, 1000, 1000, 1000]), [1000] * 4
    good = with_mates([(0, 2, 600), (2, 4, 600)], lens)
    reference_unitigs(arcs_of(good), None, off)
    reads = np.zeros(4, READ)
    reads["flags"][1] = A.SG_READ_CONTAINED
    faults = {
        "from": [(8, 2, 600)] + good[1:], "to": [(0, 9, 600)] + good[1:], "same read": good + [(6, 7, 10)],
        "len": [(0, 2, 1001)] + good[1:], "two out": good + [(0, 6, 100), (7, 1, 900)], "two in": good + [(6, 2, 100), (3, 7, 900)],
        "no mate": good[:3],
    }
    for name, rows in faults.items():
        with pytest.raises(Refused):
            reference_unitigs(arcs_of(rows), None, off)
    with pytest.raises(Refused):
        reference_unitigs(arcs_of(good, flags=A.SG_ARC_REDUCED), None, off)
    with pytest.raises(Refused):
        reference_unitigs(arcs_of(good), reads, off)
    # the same faults in arcs that are not unique count for nothing
    for rows in faults.values():
        assert len(reference_unitigs(arcs_of(rows, unique=0), None, off)[0]) == 4


def test_reference_sequences_on_a_line():
    rng = np.random.default_rng(0)
    genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), 2200)
    reads = [genome[0:1000], _COMPLEMENT[genome[600:1600][::-1]], genome[1200:2200]]
    off = offsets_of([1000] * 3)
    arcs = arcs_of(with_mates([(0, 3, 600), (3, 4, 600)], [1000] * 3))
    unitigs, path, _ = reference_unitigs(arcs, None, off)
    seq, seq_off = reference_sequences(unitigs, path, np.concatenate(reads), off)
    assert seq.tobytes() == genome.tobytes() and seq_off.tolist() == [0, 2200]
    bad = path.copy()
    bad["end"][1] = 900
    with pytest.raises(Refused):
        reference_sequences(unitigs, bad, np.concatenate(reads), off)


# ---- what the library refuses before it launches anything: no device needed ----------------------------------------------------
def test_bad_arguments_need_no_device():
    from kmerutils_amd import build, lib
    build.build()
    L = lib.load()
    assert STEP.itemsize == 16 and UNITIG.itemsize == 32 and PLACE.itemsize == 16
    arcs, off = arcs_of(with_mates([(0, 2, 600)], [1000, 1000])), offsets_of([1000, 1000])
    unitigs, path, place = np.zeros(2, UNITIG), np.zeros(2, STEP), np.zeros(2, PLACE)
    n_steps, total = C.c_uint64(7), C.c_uint64(7)
    assert L.kmu_sg_unitigs(None, arcs.ctypes.data, 2, None, off.ctypes.data, 2, A.MEM_HOST, unitigs.ctypes.data, path.ctypes.data,
                            place.ctypes.data, C.byref(n_steps), C.byref(total)) == A.E_BAD_ARG
    assert b"null" in L.kmu_last_error(None)
    bases, seq, seq_off = np.zeros(2000, np.uint8), np.zeros(16, np.uint8), np.zeros(3, np.uint64)
    assert L.kmu_sg_unitig_seqs(None, unitigs.ctypes.data, 2, path.ctypes.data, 2, bases.ctypes.data, off.ctypes.data, 2, A.MEM_HOST,
                                seq_off.ctypes.data, seq.ctypes.data, 16, C.byref(total)) == A.E_BAD_ARG
    assert n_steps.value == 7 and total.value == 7
    assert not unitigs.view(np.uint32).any() and not path.view(np.uint32).any() and not place.view(np.uint32).any() and not seq.any()

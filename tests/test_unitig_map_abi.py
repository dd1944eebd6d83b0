"""-m "not gpu": the unitig map without a device.  reference_unitig_chains, a sequential restatement of the contract of
kmu_sg_unitig_chains in include/kmu.h, which the device tests compare against; `Builder`, layouts and containment records written by
hand; `mix`, every shape the contract names in one layout; `planted_genome`, reads at known places of a genome with their layout
and their containment records (inset from the true overlap ends on the same diagonal, as seed extents are); hand cases whose
answers are written out; and the refusals the library makes before it needs a context."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import CHAIN, Refused, offsets_of  # noqa: E402
from test_unitigs_abi import PLACE, STEP, UNITIG, reference_sequences  # noqa: E402

NONE = A.SG_NONE
STATS = A.UM_STATS
A_CONT, B_CONT = A.SG_A_CONTAINED, A.SG_B_CONTAINED


def reference_unitig_chains(unitigs, path, place, chains, classes, offsets):
    """(records, stats) of the contract: the faults, then the layout reads, then the winner of every contained read"""
    off = [int(x) for x in offsets]
    n_reads = len(off) - 1
    length = [off[r + 1] - off[r] for r in range(n_reads)]
    U, P, PL = np.asarray(unitigs).tolist(), np.asarray(path).tolist(), np.asarray(place).tolist()
    rows = [] if chains is None else np.asarray(chains).tolist()
    cls = [] if classes is None else [int(x) for x in classes]
    for first, ln, n, _, _, _ in U:
        if first + n > len(P) or ln >= 1 << 32:
            raise Refused("unitig (%d, %d, %d)" % (first, ln, n))
    for read, strand, end in P:
        if read >= n_reads or strand > 1 or end == 0:
            raise Refused("step (%d, %d, %d)" % (read, strand, end))
    for r, (u, rank, s, _) in enumerate(PL):
        if u == NONE:
            continue
        if u >= len(U) or rank >= U[u][2]:
            raise Refused("place %d" % r)
        read, strand, end = P[U[u][0] + rank]
        if read != r or strand != s or end > U[u][1]:
            raise Refused("place %d and its step" % r)
    for x, row in enumerate(rows):
        if cls[x] not in (A_CONT, B_CONT):
            continue
        a, b, s, _, _, _, a_start, a_end, b_start, b_end = row
        if a >= n_reads or b >= n_reads or s > 1 or a_start > a_end or b_start > b_end or a_end > length[a] or b_end > length[b]:
            raise Refused("record %d" % x)

    def step_of(r):
        u, rank = PL[r][0], PL[r][1]
        return P[U[u][0] + rank]

    best = {}
    for x, row in enumerate(rows):
        if cls[x] not in (A_CONT, B_CONT):
            continue
        a, b, s, _, _, _, a_start, a_end, b_start, b_end = row
        c, g, cs, ce, gs, ge = (a, b, a_start, a_end, b_start, b_end) if cls[x] == A_CONT else (b, a, b_start, b_end, a_start, a_end)
        if PL[c][0] != NONE or PL[g][0] == NONE:
            continue
        _, sg, e_g = step_of(g)
        a0 = e_g - length[g] + (length[g] - ge if sg else gs)
        if a0 < 0:
            continue
        if c not in best or ce - cs > best[c][0]:  # ascending x: the first of the longest stays
            best[c] = (ce - cs, (PL[g][0], c, sg ^ s, 1, x, g, a0, a0 + ge - gs, cs, ce))
    out, stats = [], dict.fromkeys(STATS, 0)
    for r in range(n_reads):
        if PL[r][0] != NONE:
            _, s, e = step_of(r)
            t = min(length[r], e)
            out.append((PL[r][0], r, s, 0, NONE, NONE, e - t, e, 0 if s else length[r] - t, t if s else length[r]))
            stats["n_layout"] += 1
        elif r in best:
            out.append(best[r][1])
            stats["n_contained"] += 1
        else:
            stats["n_unplaced"] += 1
    return (np.array(out, CHAIN) if out else np.zeros(0, CHAIN)), stats


# ---- layouts and records by hand ---------------------------------------------------------------------------------------------------
class Builder:
    """a layout written down read by read"""

    def __init__(self):
        self.lens, self.unitigs, self.path, self.place, self.chains, self.classes = [], [], [], [], [], []

    def read(self, length):
        """a read on no unitig; returns its id"""
        self.lens.append(length)
        self.place.append((NONE, 0, 0, 0))
        return len(self.lens) - 1

    def unitig(self, steps, length=None, circular=False):
        """steps: (read length, strand, end); the reads are made here.  Returns their ids"""
        u, first, ids = len(self.unitigs), len(self.path), []
        for rank, (ln, s, end) in enumerate(steps):
            r = self.read(ln)
            self.place[r] = (u, rank, s, 0)
            self.path.append((r, s, end))
            ids.append(r)
        self.unitigs.append((first, steps[-1][2] if length is None else length, len(steps), A.SG_UNITIG_CIRCULAR if circular else 0, min(ids), 0))
        return ids

    def line(self, n, seed, length=1000, step=400):
        rng = np.random.default_rng(seed)
        return self.unitig([(length, int(rng.integers(0, 2)), length + i * step) for i in range(n)])

    def record(self, cls, a, b, strand, a_start, a_end, b_start, b_end):
        self.chains.append((a, b, strand, 7, 3, 9, a_start, a_end, b_start, b_end))
        self.classes.append(cls)
        return len(self.chains) - 1

    def contain(self, c, g, cs, ce, gs, ge, strand=0, as_a=True):
        """read c lies in read g: an A_CONTAINED record with c as read_a, or a B_CONTAINED record with c as read_b"""
        return self.record(A_CONT, c, g, strand, cs, ce, gs, ge) if as_a else self.record(B_CONT, g, c, strand, gs, ge, cs, ce)

    def arrays(self, copies=1):
        """(unitigs, path, place, chains, classes, offsets) of `copies` copies of the layout side by side"""
        n_reads, n_u, n_s = len(self.lens), len(self.unitigs), len(self.path)
        unitigs, path, place = np.array(self.unitigs * copies, UNITIG), np.array(self.path * copies, STEP), np.array(self.place * copies, PLACE)
        chains = np.array(self.chains * copies, CHAIN) if self.chains else np.zeros(0, CHAIN)
        classes = np.array(self.classes * copies, np.uint8)
        k_u, k_s, k_r, k_c = (np.repeat(np.arange(copies), n) for n in (n_u, n_s, n_reads, len(self.chains)))
        unitigs["first"] += (k_u * n_s).astype(np.uint64)
        unitigs["min_read"] += (k_u * n_reads).astype(np.uint32)
        path["read"] += (k_s * n_reads).astype(np.uint32)
        placed = place["unitig"] != NONE
        place["unitig"][placed] += (k_r * n_u).astype(np.uint32)[placed]
        if len(chains):
            chains["read_a"] += (k_c * n_reads).astype(np.uint32)
            chains["read_b"] += (k_c * n_reads).astype(np.uint32)
        return unitigs, path, place, chains, classes, offsets_of(self.lens * copies)


@functools.lru_cache(maxsize=None)
def mix():
    """every shape the contract names in one layout: (builder, names) with names[...] the reads the tests ask about"""
    b, ids = Builder(), {}
    for n in (1, 2, 64, 65):
        ids["line%d" % n] = b.line(n, seed=n)
    ids["rev"] = b.unitig([(900, 1, 900), (1000, 1, 1300), (800, 0, 1700)])
    ids["circle"] = b.unitig([(1000, 0, 300), (1000, 1, 600), (1000, 0, 900), (1000, 1, 1200), (1000, 0, 1500)], circular=True)
    ids["long"] = b.unitig([(500, 0, 500), (2000, 1, 900), (700, 0, 1300)])
    g0, g1 = ids["line64"][10], ids["line64"][11]
    # two containers of equal overlap: the smaller record index wins; a dovetail and an internal record of the same reads are not looked at
    c = ids["tie"] = b.read(400)
    b.record(A.SG_DOVETAIL, c, g0, 0, 0, 400, 0, 400)
    ids["tie_x"] = b.contain(c, g1, 5, 395, 105, 495)
    b.contain(c, g0, 5, 395, 505, 895)
    b.record(A.SG_INTERNAL, c, g1, 0, 0, 400, 600, 1000)
    # the same read as read_a of one record and as read_b of another, which is longer and wins
    c = ids["both"] = b.read(500)
    b.contain(c, g0, 10, 300, 200, 490, as_a=True)
    ids["both_x"] = b.contain(c, g1, 0, 500, 250, 750, as_a=False)
    # a container on strand 1 with the record's strand 0 and 1, and one on strand 0 with the record's strand 1
    r1 = ids["rev"][1]
    for name, g, s in (("g1s0", r1, 0), ("g1s1", r1, 1), ("g0s1", ids["rev"][2], 1)):
        ids[name] = b.read(300)
        b.contain(ids[name], g, 3, 297, 203, 497, strand=s, as_a=name != "g1s1")
    # a container that is itself contained: unplaced
    ids["deep"] = b.read(200)
    b.contain(ids["deep"], ids["tie"], 0, 200, 100, 300)
    # the longest candidate projects below 0 (the first read of the circle: 300 - 1000 + 100), the next best wins
    c = ids["below"] = b.read(450)
    b.contain(c, ids["circle"][0], 0, 450, 100, 550)
    ids["below_x"] = b.contain(c, ids["circle"][2], 20, 440, 520, 940)
    # exactly at 0, on a reverse container: 600 - 1000 + (1000 - 600) = 0
    c = ids["zero"] = b.read(350)
    b.contain(c, ids["circle"][1], 0, 350, 250, 600, strand=1)
    # a later read longer than everything before it as a container: a_start = 900 - 2000 + (2000 - 700) = 200
    c = ids["inlong"] = b.read(250)
    b.contain(c, ids["long"][1], 0, 250, 450, 700, as_a=False)
    # a placed read named as contained is not a contained read; records of other classes may hold anything
    b.contain(g0, g1, 0, 1000, 0, 1000)
    b.record(A.SG_SKIP, 1 << 30, 1 << 30, 5, 9, 1, 9, 1)
    ids["alone"] = b.read(100)  # no record at all
    return b, ids


def faulty_cases():
    """name -> the arrays of the mix with one fault of the contract planted"""
    b, ids = mix()
    out = {}

    def plant(name, which, index, field, value):
        arrays = [x.copy() for x in b.arrays()]
        arrays[which][field][index] = value
        out[name] = tuple(arrays)
    n_reads, n_steps, n_u = len(b.lens), len(b.path), len(b.unitigs)
    tie_x, r = ids["tie_x"], ids["line64"][5]
    rank = b.place[r][1]
    plant("unitig: slice beyond the steps", 0, n_u - 1, "first", n_steps - 2)
    plant("unitig: n_reads beyond the steps", 0, 2, "n_reads", n_steps)
    plant("unitig: len 2^32", 0, 3, "len", 1 << 32)
    plant("step: read out of range", 1, 7, "read", n_reads)
    plant("step: strand 2", 1, 9, "strand", 2)
    plant("step: end 0", 1, 11, "end", 0)
    plant("step: end above len", 1, b.unitigs[2][0] + 63, "end", b.unitigs[2][1] + 1)
    plant("place: unitig out of range", 2, r, "unitig", n_u)
    plant("place: rank out of range", 2, r, "rank", 64)
    plant("place: another read's step", 2, r, "rank", rank + 1)
    plant("place: the other strand", 2, r, "strand", b.place[r][2] ^ 1)
    plant("record: read_a out of range", 3, tie_x, "read_a", n_reads)
    plant("record: read_b out of range", 3, tie_x, "read_b", 0xFFFFFFFF)
    plant("record: strand 2", 3, tie_x, "strand", 2)
    plant("record: start above end", 3, tie_x, "a_start", 396)
    plant("record: b start above end", 3, tie_x, "b_start", 496)
    plant("record: a_end above the read", 3, tie_x, "a_end", 401)
    plant("record: b_end above the read", 3, tie_x, "b_end", 1001)
    return out


# ---- a genome with reads at known places -------------------------------------------------------------------------------------------
_LUT = np.frombuffer(b"ACGT", np.uint8)


def noisy_copy(rng, piece, rate):
    """(copy, where): the codes of `piece` with substitutions, deletions and insertions at `rate` in all, and where[j], the place in
    the copy of the piece's base j (where[len(piece)] is the copy's length)"""
    out, where = [], np.zeros(len(piece) + 1, np.int64)
    for j, x in enumerate(piece.tolist()):
        where[j] = len(out)
        u = rng.random() if rate else 1.0
        if u < rate / 3:
            out.append((x + 1 + int(rng.integers(0, 3))) % 4)
        elif u < 2 * rate / 3:
            pass
        elif u < rate:
            out += [x, int(rng.integers(0, 4))]
        else:
            out.append(x)
    where[len(piece)] = len(out)
    return np.array(out, np.int64), where


def planted_genome(seed, circular=False, rate=0.0, n_genome=3000, read_len=600, step=150, cont_len=320, cont_step=32, inset=3, ends=0):
    """A genome of n_genome bases; layout reads of read_len bases every `step` bases, contained reads of cont_len bases every
    cont_step bases (and `ends` more at each end of a linear genome), all on random strands, every read a noisy copy at `rate`.  The
    layout, the containment records (one per layout read that covers the contained read, inset by `inset` template bases) and the
    template the unitig should be are written from the known places.  Returns a dict: bases, offsets, unitigs, path, place, chains,
    classes, template (ASCII), n_layout."""
    rng = np.random.default_rng(seed)
    genome = rng.integers(0, 4, n_genome)
    doubled = np.concatenate([genome, genome])
    n_layout = n_genome // step if circular else (n_genome - read_len) // step + 1
    starts = [(i * step, read_len) for i in range(n_layout)]
    span = n_genome if circular else starts[-1][0] + read_len
    qs = list(range(0, span - (0 if circular else cont_len) + (0 if circular else 1), cont_step))
    if not circular:
        qs += [0] * ends + [span - cont_len] * ends
    starts += [(q, cont_len) for q in qs]
    reads = []  # (start, template length, strand, oriented copy, where)
    for i, (p, t) in enumerate(starts):
        copy, where = noisy_copy(rng, doubled[p:p + t], rate)
        reads.append((p, t, 0 if i == 0 else int(rng.integers(0, 2)), copy, where))
    lens = [len(r[3]) for r in reads]
    bases = np.concatenate([_LUT[(3 - r[3])[::-1]] if r[2] else _LUT[r[3]] for r in reads])

    def forward(r, lo, hi):
        """the oriented range [lo, hi) of read r in the read's own coordinates"""
        return (lens[r] - hi, lens[r] - lo) if reads[r][2] else (lo, hi)
    path, end = [], 0
    for i in range(n_layout):
        _, t, s, _, where = reads[i]
        end += lens[i] - int(where[t - step]) if (i or circular) else lens[i]
        path.append((i, s, end))
    unitigs = np.array([(0, end, n_layout, A.SG_UNITIG_CIRCULAR if circular else 0, 0, 0)], UNITIG)
    place = np.array([(0, i, reads[i][2], 0) if i < n_layout else (NONE, 0, 0, 0) for i in range(len(reads))], PLACE)
    rows, classes = [], []
    for c in range(n_layout, len(reads)):
        q, t = reads[c][0], reads[c][1]
        for g in range(n_layout):
            for shift in ((0, n_genome) if circular else (0,)):
                lo, hi = q + shift + inset, q + shift + t - inset
                p = reads[g][0]
                if not (p <= lo - inset and hi + inset <= p + read_len):
                    continue
                cs, ce = forward(c, int(reads[c][4][inset]), int(reads[c][4][t - inset]))
                gs, ge = forward(g, int(reads[g][4][lo - p]), int(reads[g][4][hi - p]))
                # read_a < read_b, as the self-join writes its records: g < c always here, so c is read_b of a B_CONTAINED record
                rows.append((g, c, reads[c][2] ^ reads[g][2], 0, 0, 0, gs, ge, cs, ce))
                classes.append(B_CONT)
    first = (read_len - step) if circular else 0
    template = _LUT[doubled[first:first + span]]
    return dict(bases=bases, offsets=offsets_of(lens), unitigs=unitigs, path=np.array(path, STEP), place=place,
                chains=np.array(rows, CHAIN), classes=np.array(classes, np.uint8), template=template, n_layout=n_layout)


def edit_distance(a, b):
    """unit-cost edit distance of two byte arrays, a row of the matrix at a time"""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    j = np.arange(len(b) + 1)
    row = j.copy()
    for i, x in enumerate(a.tolist(), 1):
        best = np.minimum(row[1:] + 1, row[:-1] + (b != x))
        row = np.minimum.accumulate(np.concatenate([[i], best]) - j) + j
    return int(row[-1])


# ---- hand cases --------------------------------------------------------------------------------------------------------------------
def by_read(records):
    return {int(r["read_b"]): tuple(int(x) for x in r) for r in records}


def test_hand_cases_of_the_mix():
    b, ids = mix()
    records, stats = reference_unitig_chains(*b.arrays())
    got = by_read(records)
    assert records["read_b"].tolist() == sorted(got) and len(got) == len(records)
    n_layout = 1 + 2 + 64 + 65 + 3 + 5 + 3
    assert stats == dict(n_layout=n_layout, n_contained=8, n_unplaced=2) and len(records) == n_layout + 8
    assert ids["deep"] not in got and ids["alone"] not in got
    u64, u_rev, u_circle, u_long = 2, 4, 5, 6
    g0, g1 = ids["line64"][10], ids["line64"][11]
    e0, e1 = 1000 + 10 * 400, 1000 + 11 * 400
    s0, s1 = b.place[g0][2], b.place[g1][2]
    # the layout reads: whole reads on the line, the tail of the read where the step ends before the read's length
    assert got[g0] == (u64, g0, s0, 0, NONE, NONE, e0 - 1000, e0, 0, 1000)
    assert got[ids["circle"][0]] == (u_circle, ids["circle"][0], 0, 0, NONE, NONE, 0, 300, 700, 1000)
    assert got[ids["circle"][1]] == (u_circle, ids["circle"][1], 1, 0, NONE, NONE, 0, 600, 0, 600)
    assert got[ids["circle"][3]] == (u_circle, ids["circle"][3], 1, 0, NONE, NONE, 200, 1200, 0, 1000)
    assert got[ids["long"][1]] == (u_long, ids["long"][1], 1, 0, NONE, NONE, 0, 900, 0, 900)
    assert got[ids["rev"][0]] == (u_rev, ids["rev"][0], 1, 0, NONE, NONE, 0, 900, 0, 900)
    # the contained reads
    os1 = 1000 - 495 if s1 else 105
    assert got[ids["tie"]] == (u64, ids["tie"], s1, 1, ids["tie_x"], g1, e1 - 1000 + os1, e1 - 1000 + os1 + 390, 5, 395)
    os1 = 1000 - 750 if s1 else 250
    assert got[ids["both"]] == (u64, ids["both"], s1, 1, ids["both_x"], g1, e1 - 1000 + os1, e1 - 1000 + os1 + 500, 0, 500)
    r1 = ids["rev"][1]  # strand 1, end 1300, 1000 bases: os = 1000 - 497
    assert got[ids["g1s0"]][:4] == (u_rev, ids["g1s0"], 1, 1) and got[ids["g1s0"]][5:] == (r1, 803, 1097, 3, 297)
    assert got[ids["g1s1"]][:4] == (u_rev, ids["g1s1"], 0, 1) and got[ids["g1s1"]][5:] == (r1, 803, 1097, 3, 297)
    assert got[ids["g0s1"]][:4] == (u_rev, ids["g0s1"], 1, 1) and got[ids["g0s1"]][5:] == (ids["rev"][2], 900 + 203, 900 + 497, 3, 297)
    assert got[ids["below"]] == (u_circle, ids["below"], 0, 1, ids["below_x"], ids["circle"][2], 420, 840, 20, 440)
    assert got[ids["zero"]] == (u_circle, ids["zero"], 0, 1, ids["below_x"] + 1, ids["circle"][1], 0, 350, 0, 350)
    assert got[ids["inlong"]][2:] == (1, 1, got[ids["inlong"]][4], ids["long"][1], 200, 450, 0, 250)


def test_copies_of_the_mix_are_the_mix_shifted():
    b, _ = mix()
    one, _ = reference_unitig_chains(*b.arrays())
    two, stats = reference_unitig_chains(*b.arrays(2))
    assert len(two) == 2 * len(one) and stats["n_unplaced"] == 4
    second = two[len(one):].copy()
    second["read_a"] -= len(b.unitigs)
    second["read_b"] -= len(b.lens)
    cont = second["score"] == 1
    second["n_seeds"][cont] -= len(b.chains)
    second["n_anchors"][cont] -= len(b.lens)
    assert second.tobytes() == one.tobytes() and two[:len(one)].tobytes() == one.tobytes()


def test_without_records_only_the_layout_is_mapped():
    b, _ = mix()
    unitigs, path, place, _, _, off = b.arrays()
    records, stats = reference_unitig_chains(unitigs, path, place, None, None, off)
    assert stats == dict(n_layout=143, n_contained=0, n_unplaced=len(b.lens) - 143) and (records["score"] == 0).all()


@pytest.mark.parametrize("fault", sorted(faulty_cases()))
def test_every_fault_is_refused(fault):
    with pytest.raises(Refused):
        reference_unitig_chains(*faulty_cases()[fault])


@pytest.mark.parametrize("circular", [False, True])
def test_planted_genome_coordinates_are_exact_without_errors(circular):
    """every record of the map names two equal strings: the coordinate arithmetic of the builder and of the reference agree"""
    g = planted_genome(5, circular)
    seq, seq_off = reference_sequences(g["unitigs"], g["path"], g["bases"], g["offsets"])
    assert seq.tobytes() == g["template"].tobytes() and seq_off.tolist() == [0, len(seq)]
    records, stats = reference_unitig_chains(g["unitigs"], g["path"], g["place"], g["chains"], g["classes"], g["offsets"])
    assert stats["n_layout"] == g["n_layout"] and stats["n_contained"] > 80
    # on the circle the reads that straddle the place where the unitig was cut open have no container that projects to 0 or above
    assert stats["n_unplaced"] == (9 if circular else 0)
    off = g["offsets"].astype(np.int64)
    comp = np.full(256, ord("N"), np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    for r in records:
        a = seq[int(r["a_start"]):int(r["a_end"])]
        b = g["bases"][off[r["read_b"]] + int(r["b_start"]):off[r["read_b"]] + int(r["b_end"])]
        assert a.tobytes() == (comp[b[::-1]] if r["strand"] else b).tobytes() and len(a) > 100, r


def test_edit_distance_by_hand():
    s = lambda t: np.frombuffer(t, np.uint8)  # noqa: E731
    assert edit_distance(s(b"ACGT"), s(b"ACGT")) == 0 and edit_distance(s(b"ACGT"), s(b"AGT")) == 1
    assert edit_distance(s(b"AAAA"), s(b"TTTT")) == 4 and edit_distance(s(b""), s(b"ACG")) == 3 and edit_distance(s(b"GATTACA"), s(b"GCATGCT")) == 4


def test_noisy_copy_keeps_track_of_places():
    rng = np.random.default_rng(3)
    piece = rng.integers(0, 4, 500)
    copy, where = noisy_copy(rng, piece, 0.05)
    assert where[0] == 0 and where[-1] == len(copy) and (np.diff(where) >= 0).all() and (np.diff(where) <= 2).all()
    assert 0 < edit_distance(copy, piece) <= 40
    same, where = noisy_copy(rng, piece, 0.0)
    assert same.tolist() == piece.tolist() and where.tolist() == list(range(501))


# ---- the library without a device --------------------------------------------------------------------------------------------------
def test_symbol_bindings_and_struct_sizes():
    from kmerutils_amd import build, lib
    build.build()
    L = lib.load()
    assert "kmu_sg_unitig_chains" in lib.SYMBOLS and len(L.kmu_sg_unitig_chains.argtypes) == 16
    assert C.sizeof(A.UmParams) == 8 and C.sizeof(A.UmStats) == np.dtype(A.UM_STATS_DTYPE).itemsize == 24
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmu.h")).read()
    assert "int kmu_sg_unitig_chains(kmu_ctx *ctx" in header and "} kmu_um_params;" in header and "} kmu_um_stats;" in header


def test_bad_arguments_need_no_device():
    from kmerutils_amd import build, lib
    build.build()
    L = lib.load()
    b, _ = mix()
    unitigs, path, place, chains, classes, off = b.arrays()
    n_reads = len(b.lens)
    out, stats, n_out = np.zeros(n_reads, CHAIN), A.UmStats(7, 7, 7), C.c_uint64(7)

    def call(**kw):
        a = dict(ctx=None, unitigs=unitigs.ctypes.data, n_unitigs=len(unitigs), path=path.ctypes.data, n_steps=len(path), place=place.ctypes.data,
                 chains=chains.ctypes.data, classes=classes.ctypes.data, n_chains=len(chains), off=off.ctypes.data, n_reads=n_reads,
                 p=C.byref(A.UmParams(0, 0)), mem=A.MEM_HOST, out=out.ctypes.data, stats=C.byref(stats), n_out=C.byref(n_out))
        a.update(kw)
        return L.kmu_sg_unitig_chains(*a.values())
    null = C.POINTER(A.UmParams)()
    bad = [(dict(p=null), b"null"), (dict(off=None), b"null"), (dict(stats=None), b"null"), (dict(n_out=None), b"null"),
           (dict(unitigs=None), b"null"), (dict(path=None), b"null"), (dict(place=None), b"null"), (dict(out=None), b"null"),
           (dict(chains=None), b"null"), (dict(classes=None), b"null"), (dict(p=C.byref(A.UmParams(1, 0))), b"flags"),
           (dict(p=C.byref(A.UmParams(0, 1))), b"zero"), (dict(mem=7), b"bad mem"), (dict(), b"null context")]
    for kw, word in bad:
        assert call(**kw) == A.E_BAD_ARG and word in L.kmu_last_error(None), (kw, L.kmu_last_error(None))
    assert call(n_reads=1 << 31) == A.E_UNSUPPORTED and b"2^31" in L.kmu_last_error(None)
    assert call(n_chains=1 << 32) == A.E_UNSUPPORTED and b"2^32" in L.kmu_last_error(None)
    assert [getattr(stats, k) for k in STATS] == [7] * 3 and n_out.value == 7 and not out.view(np.uint32).any()

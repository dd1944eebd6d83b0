"""The unitig layout on the device (kmu_sg_unitigs, kmu_sg_unitig_seqs and the wrappers above them) against the references of
tests/test_unitigs_abi.py: every output whole array against whole array, byte for byte, on host arrays and on resident tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import ARC, READ, Refused, offsets_of, params, planted_pile, planted_random, planted_tiling  # noqa: E402
from test_unitigs_abi import (PLACE, STEP, UNITIG, _COMPLEMENT, arcs_of, circle_arcs, hostile_graph, planted_unitigs,  # noqa: E402
                              reference_sequences, reference_unitigs, with_mates)

pytestmark = pytest.mark.gpu
TILE = 4096  # output bytes per tile of k_ut_seq_copy


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def dev(x, cols=None):
    """a numpy array of records (cols int32 columns each) or of plain numbers as a resident tensor holding the same bits"""
    import torch
    if x is None:
        return None
    x = np.ascontiguousarray(x)
    if cols:
        return torch.from_numpy(x.view(np.int32).reshape(-1, cols).copy()).cuda()
    return torch.from_numpy(x.view(np.int64 if x.dtype == np.uint64 else x.dtype).copy()).cuda()


def host(x, dtype=None):
    x = x.cpu().numpy()
    return x.reshape(-1).view(dtype) if dtype is not None else x


def same(got, want, what):
    for name, g, w in zip(("unitigs", "path", "place", "seq", "seq_offsets"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g[:8], w[:8])


def check(ctx, arcs, reads, offsets, want=None, what=""):
    """both modes of sg_unitigs against the reference; returns the reference's outputs"""
    want = want if want is not None else reference_unitigs(arcs, reads, offsets)
    same(ctx.sg_unitigs(arcs, reads, offsets), want, what + " host")
    got = ctx.sg_unitigs(dev(arcs, 8), dev(reads, 4), dev(offsets))
    same((host(got[0], UNITIG), host(got[1], STEP), host(got[2], PLACE)), want, what + " device")
    return want


def check_seqs(ctx, unitigs, path, bases, offsets, what=""):
    want = reference_sequences(unitigs, path, bases, offsets)
    same(ctx.sg_unitig_seqs(unitigs, path, bases, offsets), want, what + " host")
    got = ctx.sg_unitig_seqs(dev(unitigs, 8), dev(path, 4), dev(bases), dev(offsets))
    same((host(got[0]), host(got[1]).view(np.uint64)), want, what + " device")
    return want


def forest(sizes, circular, seed, zero_every=0):
    """paths and circles of the given numbers of reads with shuffled ids and strands, as arcs with their mates in shuffled order;
    zero_every: every so-many-th arc and its mate have len 0.  Returns (arcs, offsets)"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    ids, flip, lens = rng.permutation(n), rng.integers(0, 2, n), rng.integers(500, 600, n)
    rows, at = [], 0
    for size, cyc in zip(sizes, circular):
        vs = [2 * int(ids[at + i]) + int(flip[at + i]) for i in range(size)]
        at += size
        rows += [(vs[i], vs[(i + 1) % size], int(rng.integers(150, 250))) for i in range(size if cyc else size - 1)]
    arcs = arcs_of(with_mates(rows, lens))
    if zero_every:
        pairs = np.arange(len(rows))[zero_every - 1::zero_every]
        arcs["len"][2 * pairs] = arcs["len"][2 * pairs + 1] = 0
    return arcs[rng.permutation(len(arcs))], offsets_of(lens)


# ---- the cases of tests/test_unitigs_abi.py, through overlap_graph ------------------------------------------------------------------
@pytest.mark.parametrize("name,arg", [("tiling", 0), ("tiling", 3), ("random", None), ("pile", 65)])
def test_planted_layouts(ctx, name, arg):
    (arcs, reads, offsets, _), want = planted_unitigs(name, arg)
    case = {"tiling": planted_tiling, "random": planted_random, "pile": planted_pile}[name]
    got = case(arg) if arg is not None else case()
    d_arcs, _, _, d_reads = minimizer.overlap_graph(ctx, got[0], None, got[1], **got[3])
    assert d_arcs.tobytes() == arcs.tobytes() and d_reads.tobytes() == reads.tobytes()
    check(ctx, d_arcs, d_reads, offsets, want, name)
    same(minimizer.unitig_paths(ctx, d_arcs, d_reads, offsets), want, name + " wrapper")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hostile_graphs(ctx, seed):
    arcs, reads, offsets, chains = hostile_graph(seed)
    d_arcs, _, _, d_reads = minimizer.overlap_graph(ctx, chains, None, offsets, **params(fuzz=20))
    assert d_arcs.tobytes() == arcs.tobytes() and d_reads.tobytes() == reads.tobytes()
    want = check(ctx, d_arcs, d_reads, offsets, what="hostile")
    assert int((want[0]["n_reads"] > 1).sum()) == 3


def test_hand_cases(ctx):
    off = offsets_of([1000, 1000, 1000])
    want = check(ctx, arcs_of(with_mates([(0, 2, 100), (2, 4, 100)], [1000] * 3)), None, off, what="the smoke line")
    assert want[0].tolist() == [(0, 1200, 3, 0, 0, 0)]
    want = check(ctx, np.zeros(0, ARC), None, off, what="no arcs")
    assert len(want[0]) == 3
    none = np.zeros(3, READ)
    none["flags"] = A.SG_READ_CONTAINED
    want = check(ctx, np.zeros(0, ARC), none, off, what="every read contained")
    assert len(want[0]) == 0 and len(want[1]) == 0 and want[2]["unitig"].tolist() == [A.SG_NONE] * 3
    for sa in (0, 1):
        for sb in (0, 1):
            check(ctx, arcs_of(with_mates([(sa, 2 + sb, 300)], [1000, 800])), None, offsets_of([1000, 800]), what="strands")
    want = check(ctx, arcs_of(with_mates([(2, 1, 200)], [500, 700])), None, offsets_of([500, 700]), what="orientation")
    assert want[1].tolist() == [(0, 0, 500), (1, 1, 900)]
    check(ctx, np.zeros(0, ARC), None, offsets_of([77]), what="one read")


@pytest.mark.parametrize("n", [3, 4, 64, 65])
def test_circles(ctx, n):
    rng = np.random.default_rng(n)
    arcs, off, _ = circle_arcs(n, rng.integers(500, 600, n), rng.integers(150, 250, n), seed=n)
    want = check(ctx, arcs, None, off, what="circle")
    assert want[0]["flags"].tolist() == [A.SG_UNITIG_CIRCULAR] and tuple(want[1][0])[:2] == (0, 0)


# ---- the edges of the round count, many unitigs in one call ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1025])
def test_lines(ctx, n):
    arcs, off = forest([n], [False], seed=n)
    want = check(ctx, arcs, None, off, what="line of %d" % n)
    assert want[0]["n_reads"].tolist() == [n]


def test_many_paths_and_circles_in_one_call(ctx):
    rng = np.random.default_rng(9)
    sizes = rng.integers(1, 10, 300).tolist() + rng.integers(2, 40, 20).tolist()
    arcs, off = forest(sizes, [False] * 300 + [True] * 20, seed=10, zero_every=7)
    want = check(ctx, arcs, None, off, what="forest")
    assert len(want[0]) == 320 and int((want[0]["flags"] == A.SG_UNITIG_CIRCULAR).sum()) == 20
    # the order of the arcs does not matter
    same(ctx.sg_unitigs(arcs[np.random.default_rng(1).permutation(len(arcs))], None, off), want, "shuffled")
    same(ctx.sg_unitigs(arcs[::-1], None, off), want, "reversed")
    # arcs that are not unique count for nothing, whatever they hold; reduced ones among them
    junk = np.zeros(500, ARC)
    for f in ("from", "to", "len", "flags"):
        junk[f] = rng.integers(0, 1 << 32, 500)
    junk["unique"] = rng.choice([0, 2, 7], 500)
    mixed = np.concatenate([arcs, junk])
    check(ctx, mixed[rng.permutation(len(mixed))], None, off, want, "junk mixed in")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class Raw:
    """the entry point itself on prefilled outputs, host arrays or resident tensors"""

    def __init__(self, arcs, reads, offsets, device=False):
        self.device = device
        self.n_reads = len(offsets) - 1
        fill = lambda dtype: np.frombuffer(bytes([0xAB]) * (dtype.itemsize * self.n_reads), dtype).copy()  # noqa: E731
        self.outs = [fill(UNITIG), fill(STEP), fill(PLACE)]
        self.want = [x.tobytes() for x in self.outs]
        self.ins = [np.ascontiguousarray(arcs), reads, np.asarray(offsets).astype(np.uint64)]
        if device:
            self.ins = [dev(self.ins[0], 8), dev(reads, 4), dev(self.ins[2])]
            self.outs = [dev(self.outs[0], 8), dev(self.outs[1], 4), dev(self.outs[2], 4)]
        self.n_steps, self.total = C.c_uint64(12345), C.c_uint64(12345)

    def call(self, ctx, **kw):
        p = lambda x: lib._ptr(x)[0]  # noqa: E731
        args = dict(ctx=ctx.h, arcs=p(self.ins[0]), n_arcs=int(self.ins[0].shape[0]), reads=p(self.ins[1]), offsets=p(self.ins[2]),
                    n_reads=self.n_reads, mem=A.MEM_DEVICE if self.device else A.MEM_HOST, unitigs=p(self.outs[0]), path=p(self.outs[1]),
                    place=p(self.outs[2]), n_steps=C.byref(self.n_steps), total=C.byref(self.total))
        args.update(kw)
        return ctx.L.kmu_sg_unitigs(*args.values())

    def untouched(self):
        got = [host(x).tobytes() if self.device else x.tobytes() for x in self.outs]
        return got == self.want and self.n_steps.value == 12345 and self.total.value == 12345


def faulty(arcs, reads, fault, at):
    """the arcs with one fault planted in unique arc number `at`; (arcs, reads)"""
    bad = arcs.copy()
    i = int(np.flatnonzero(bad["unique"] == 1)[at])
    n_v = 2 * len(reads)
    if fault == "from":
        bad["from"][i] = n_v
    elif fault == "to":
        bad["to"][i] = 0xFFFFFFFF
    elif fault == "same read":
        bad["to"][i] = bad["from"][i] ^ 1
    elif fault == "len":
        bad["len"][i] = 401
    elif fault == "reduced":
        bad["flags"][i] = A.SG_ARC_REDUCED
    elif fault == "twice":
        bad = np.concatenate([bad, bad[i:i + 1]])
    elif fault == "no mate":
        bad["unique"][i] = 0
    elif fault == "contained":
        reads = reads.copy()
        reads["flags"][int(bad["to"][i]) >> 1] = A.SG_READ_CONTAINED
    return bad, reads


@pytest.mark.parametrize("fault", ["from", "to", "same read", "len", "reduced", "twice", "no mate", "contained"])
@pytest.mark.parametrize("at", [0, 40])
def test_device_found_refusals(ctx, fault, at):
    (arcs, reads, offsets, _), want = planted_unitigs("tiling", 0)
    bad, bad_reads = faulty(arcs, reads, fault, at)
    with pytest.raises(Refused):
        reference_unitigs(bad, bad_reads, offsets)
    for device in (False, True):
        r = Raw(bad, bad_reads, offsets, device)
        assert r.call(ctx) == A.E_UNSUPPORTED and r.untouched(), (fault, at, device)
    with pytest.raises(lib.KmuError) as e:
        ctx.sg_unitigs(bad, bad_reads, offsets)
    assert e.value.code == A.E_UNSUPPORTED
    check(ctx, arcs, reads, offsets, want, "after a refusal")


def test_bad_arguments(ctx):
    (arcs, reads, offsets, _), want = planted_unitigs("tiling", 0)
    r = Raw(arcs, reads, offsets)
    for kw in (dict(offsets=None), dict(total=None), dict(unitigs=None), dict(path=None), dict(arcs=None), dict(mem=2), dict(mem=-1)):
        assert r.call(ctx, **kw) == A.E_BAD_ARG and r.untouched(), kw
    assert r.call(ctx, n_reads=1 << 31) == A.E_UNSUPPORTED and r.untouched()
    # the optional ones may be null; no reads at all is a good call
    assert r.call(ctx, n_reads=0, n_arcs=0) == A.OK and (r.total.value, r.n_steps.value) == (0, 0)
    r = Raw(arcs, reads, offsets)
    assert r.call(ctx, place=None, n_steps=None, reads=None) == A.OK and r.total.value == 1 and r.n_steps.value == 12345
    assert r.outs[0][:1].tobytes() == want[0].tobytes() and r.outs[1].tobytes() == want[1].tobytes() and r.outs[2].tobytes() == r.want[2]
    assert r.outs[0][1:].tobytes() == r.want[0][UNITIG.itemsize:]  # records beyond the count are left untouched


# ---- sequences ---------------------------------------------------------------------------------------------------------------------
def hand_layout(contribs, read_lens, seed, alphabet=b"ACGT"):
    """unitigs given as lists of contributions: step j of a unitig takes its bytes from a read of its own with a random strand"""
    rng = np.random.default_rng(seed)
    n = sum(len(c) for c in contribs)
    lens = np.asarray(read_lens(n, rng), np.int64)
    bases = rng.choice(np.frombuffer(alphabet, np.uint8), int(lens.sum()))
    reads, unitigs, path, r = rng.permutation(n), np.zeros(len(contribs), UNITIG), np.zeros(n, STEP), 0
    for u, cs in enumerate(contribs):
        end = 0
        for c in cs:
            end += min(int(c), int(lens[reads[r]]))
            path[r] = (reads[r], rng.integers(0, 2), end)
            r += 1
        unitigs[u] = (r - len(cs), end, len(cs), 0, 0, 0)
    return unitigs, path, bases, offsets_of(lens)


def test_sequences_at_the_tile_edges(ctx):
    # one unitig of one step per length; then the same lengths made of many steps; then all in one call, tiles shared by unitigs
    big = lambda n, rng: np.full(n, 2 * TILE + 50)  # noqa: E731
    for length in (TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1):
        check_seqs(ctx, *hand_layout([[length]], big, seed=length), what="one step of %d" % length)
    small = lambda n, rng: rng.integers(1, 200, n)  # noqa: E731
    for length in (TILE - 1, TILE, TILE + 1):
        cs = [100] * (length // 100) + [length % 100]
        unitigs, path, bases, off = hand_layout([cs], lambda n, rng: np.full(n, 100), seed=length)
        seq, _ = check_seqs(ctx, unitigs, path, bases, off, what="steps up to %d" % length)
        assert len(seq) == length
    many = [list(np.random.default_rng(3).integers(0, 200, 1 + i % 70)) for i in range(150)]
    seq, seq_off = check_seqs(ctx, *hand_layout(many, small, seed=4), what="many")
    assert len(seq) > 3 * TILE and len(seq_off) == 151
    # n one-byte steps: n + 1 ends take one and two rounds of the 64-ary search; at 4097 the second tile's first byte lies in the last item
    for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1):
        seq, _ = check_seqs(ctx, *hand_layout([[1] * n], small, seed=n), what="%d steps of one byte" % n)
        assert len(seq) == n
    # a tile that ends on an item's end, more than 64 items of nothing before the next byte, and items of nothing behind the last byte
    gaps = [TILE] + [0] * 130 + [10] + [0] * 70
    seq, _ = check_seqs(ctx, *hand_layout([gaps], lambda n, rng: np.full(n, TILE), seed=8), what="gaps")
    assert len(seq) == TILE + 10


def test_sequences_with_contributions_of_zero(ctx):
    arcs, off = forest([5, 70, 3, 130], [False, True, False, False], seed=21, zero_every=3)
    unitigs, path, _ = check(ctx, arcs, None, off, what="zeros")
    assert (np.diff(path["end"].astype(np.int64)) == 0).sum() > 20
    bases = np.random.default_rng(2).choice(np.frombuffer(b"ACGT", np.uint8), int(off[-1]))
    check_seqs(ctx, unitigs, path, bases, off, what="zeros")
    # unitigs of nothing but zeros, and unitigs without steps, between others
    zeros = [[0, 0, 0], [50], [], [0] * 130, [7, 0, 0, 9], []]
    seq, seq_off = check_seqs(ctx, *hand_layout(zeros, lambda n, rng: np.full(n, 60), seed=5), what="all zero")
    assert seq_off.tolist() == [0, 0, 50, 50, 50, 66, 66]


def test_sequences_of_lowercase_and_other_bytes(ctx):
    layout = hand_layout([[300, 20, 300], [150]], lambda n, rng: np.full(n, 300), seed=6, alphabet=b"ACGTacgtNn-x\x00\xff")
    layout[1]["strand"][:] = [0, 1, 1, 0]
    seq, _ = check_seqs(ctx, *layout, what="bytes")
    assert {ord("N"), ord("a"), ord("t"), 0xFF} <= set(seq.tolist())
    whole = _COMPLEMENT[layout[2][::-1]]
    assert (whole[np.isin(layout[2][::-1], np.frombuffer(b"Nn-x\x00\xff", np.uint8))] == ord("N")).all()


def test_sequences_count_only_and_capacity(ctx):
    unitigs, path, bases, off = hand_layout([[100, 30], [64]], lambda n, rng: np.full(n, 100), seed=7)
    want, _ = reference_sequences(unitigs, path, bases, off)
    for device in (False, True):
        ins = [unitigs, path, bases, off]
        seq, seq_off = np.full(256, 0xAB, np.uint8), np.full(3, 0xABAB, np.uint64)
        if device:
            ins, seq, seq_off = [dev(unitigs, 8), dev(path, 4), dev(bases), dev(off)], dev(seq), dev(seq_off)
        p = lambda x: lib._ptr(x)[0]  # noqa: E731
        mem, total = A.MEM_DEVICE if device else A.MEM_HOST, C.c_uint64(5)
        head = (ctx.h, p(ins[0]), 2, p(ins[1]), 3, p(ins[2]), p(ins[3]), 3, mem)
        untouched = lambda: (host(seq) == 0xAB).all() and (host(seq_off).view(np.uint64) == 0xABAB).all()  # noqa: E731
        if not device:
            untouched = lambda: (seq == 0xAB).all() and (seq_off == 0xABAB).all()  # noqa: E731
        assert ctx.L.kmu_sg_unitig_seqs(*head, p(seq_off), None, 0, C.byref(total)) == A.OK and total.value == 194 and untouched()
        total.value = 5
        assert ctx.L.kmu_sg_unitig_seqs(*head, p(seq_off), p(seq), 193, C.byref(total)) == A.E_BAD_ARG and total.value == 194 and untouched()
        assert ctx.L.kmu_sg_unitig_seqs(*head, None, p(seq), 194, C.byref(total)) == A.OK
        got = host(seq) if device else seq
        assert got[:194].tobytes() == want.tobytes() and (got[194:] == 0xAB).all()
        assert ctx.L.kmu_sg_unitig_seqs(*head[:-1], 3, p(seq_off), p(seq), 256, C.byref(total)) == A.E_BAD_ARG
        assert ctx.L.kmu_sg_unitig_seqs(*head, p(seq_off), p(seq), 256, None) == A.E_BAD_ARG
        assert ctx.L.kmu_sg_unitig_seqs(ctx.h, None, 2, *head[3:], p(seq_off), p(seq), 256, C.byref(total)) == A.E_BAD_ARG


SEQ_FAULTS = {
    "slice": lambda u, s: u["first"].__setitem__(1, 3), "count": lambda u, s: u["n_reads"].__setitem__(1, 4),
    "read": lambda u, s: s["read"].__setitem__(2, 4), "strand": lambda u, s: s["strand"].__setitem__(0, 2),
    "ends decrease": lambda u, s: s["end"].__setitem__(1, 99), "contribution": lambda u, s: s["end"].__setitem__(0, 101),
    "len": lambda u, s: u["len"].__setitem__(0, 131), "first overflows": lambda u, s: u["first"].__setitem__(0, (1 << 64) - 1),
}


@pytest.mark.parametrize("fault", sorted(SEQ_FAULTS))
def test_sequence_faults_are_refused(ctx, fault):
    unitigs, path, bases, off = hand_layout([[100, 30], [64, 0]], lambda n, rng: np.full(n, 100), seed=8)
    good = check_seqs(ctx, unitigs, path, bases, off)
    bad_u, bad_s = unitigs.copy(), path.copy()
    SEQ_FAULTS[fault](bad_u, bad_s)
    if fault != "first overflows":  # (Python's integers do not wrap)
        with pytest.raises(Refused):
            reference_sequences(bad_u, bad_s, bases, off)
    seq, seq_off, total = np.full(256, 0xAB, np.uint8), np.full(3, 0xABAB, np.uint64), C.c_uint64(5)
    assert ctx.L.kmu_sg_unitig_seqs(ctx.h, bad_u.ctypes.data, 2, bad_s.ctypes.data, 4, bases.ctypes.data, off.ctypes.data, 4, A.MEM_HOST,
                                    seq_off.ctypes.data, seq.ctypes.data, 256, C.byref(total)) == A.E_UNSUPPORTED
    assert (seq == 0xAB).all() and (seq_off == 0xABAB).all()
    with pytest.raises(lib.KmuError) as e:
        ctx.sg_unitig_seqs(dev(bad_u, 8), dev(bad_s, 4), dev(bases), dev(off))
    assert e.value.code == A.E_UNSUPPORTED
    same(ctx.sg_unitig_seqs(unitigs, path, bases, off), good, "after a refusal")


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def revcomp(x):
    return _COMPLEMENT[np.asarray(x, np.uint8)[::-1]]


def test_read_unitigs_end_to_end(ctx):
    """the genome and the reads of test_read_graph_end_to_end (tests/test_gpu_string_graph.py), the same construction"""
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 6000).astype(np.uint8)
    k, w, n = 15, 5, 60
    starts = np.round(np.arange(n) * (5400 / (n - 1))).astype(np.int64)
    order = rng.permutation(n)
    lut, parts = np.frombuffer(b"ACGT", np.uint8), []
    for i in order:
        piece = genome[starts[i]:starts[i] + 600]
        parts.append(lut[(3 - piece)[::-1]] if rng.integers(0, 2) else lut[piece])
    bases, offsets = np.concatenate(parts), offsets_of([600] * n)
    p = params(min_overlap=100, fuzz=10)
    got = minimizer.read_unitigs(ctx, dev(bases), dev(offsets), k, w, **p)
    assert all(x.is_cuda for x in got)
    unitigs, path, place = host(got[0], UNITIG), host(got[1], STEP), host(got[2], PLACE)
    seq, seq_off = host(got[3]), host(got[4]).view(np.uint64)
    assert unitigs.tolist() == [(0, 6000, n, 0, 0, 0)] and len(path) == n and seq_off.tolist() == [0, 6000]
    assert path["read"].tolist() in ([int(np.flatnonzero(order == i)[0]) for i in range(n)], [int(np.flatnonzero(order == i)[0]) for i in range(n)][::-1])
    assert seq.tobytes() in (lut[genome].tobytes(), revcomp(lut[genome]).tobytes())
    # host arrays give the same
    same(minimizer.read_unitigs(ctx, bases, offsets, k, w, **p), (unitigs, path, place, seq, seq_off), "host")
    names = ["r%d" % i for i in range(n)]
    lines = minimizer.unitig_gfa_lines(unitigs, path, seq, seq_off, names)
    assert lines[0] == "S\tutg000000l\t%s\tLN:i:6000" % seq.tobytes().decode() and len(lines) == 1 + n
    first = path[0]
    assert lines[1] == "a\tutg000000l\t0\tr%d\t%s\t600" % (first["read"], "+-"[first["strand"]])
    assert lines[2].split("\t")[2] == "600" and lines[2].split("\t")[5] == str(int(path["end"][1]) - 600)


def test_circular_genome_end_to_end(ctx):
    """30 reads of 600 at step 100 round a circular genome of 3 000 bases; the chain records are built on the host with exact
    coordinates, the graph, the unitig and its bases come from the device"""
    from test_string_graph_abi import records
    rng = np.random.default_rng(123)
    lut = np.frombuffer(b"ACGT", np.uint8)
    genome = lut[rng.integers(0, 4, 3000)]
    n = 30
    ids, flip = rng.permutation(n), rng.integers(0, 2, n)
    parts, rows = [None] * n, []
    for i in range(n):
        piece = np.concatenate([genome, genome])[100 * i:100 * i + 600]
        parts[ids[i]] = revcomp(piece) if flip[i] else piece
    for i in range(n):
        for d in range(1, 6):  # read i + d starts d * 100 after read i: they share 600 - 100 d bases
            j, share = (i + d) % n, 600 - 100 * d
            a_rng = (0, share) if flip[i] else (600 - share, 600)  # the shared stretch on read i as stored, on read j as stored
            b_rng = (600 - share, 600) if flip[j] else (0, share)
            a, b = (i, j) if ids[i] < ids[j] else (j, i)
            (a0, a1), (b0, b1) = (a_rng, b_rng) if a == i else (b_rng, a_rng)
            rows.append((int(ids[a]), int(ids[b]), int(flip[a] ^ flip[b]), a0, a1, b0, b1))
    bases, offsets = np.concatenate(parts), offsets_of([600] * n)
    arcs, _, _, reads = minimizer.overlap_graph(ctx, records(rows), None, offsets, **params(min_overlap=100))
    assert int(arcs["unique"].sum()) == 2 * n and not reads["flags"].any()
    unitigs, path, place = check(ctx, arcs, reads, offsets, what="circular genome")
    assert unitigs.tolist() == [(0, 3000, n, A.SG_UNITIG_CIRCULAR, 0, 0)]
    seq, seq_off = check_seqs(ctx, unitigs, path, bases, offsets, what="circular genome")
    doubled = (np.concatenate([genome, genome]).tobytes(), np.concatenate([revcomp(genome), revcomp(genome)]).tobytes())
    assert len(seq) == 3000 and any(seq.tobytes() in d for d in doubled)
    assert minimizer.unitig_gfa_lines(unitigs, path, seq, seq_off, ["r%d" % i for i in range(n)])[0].startswith("S\tutg000000c\t")


def test_the_kernels_that_ran(ctx):
    (arcs, reads, offsets, _), want = planted_unitigs("tiling", 0)
    bases = np.random.default_rng(0).choice(np.frombuffer(b"ACGT", np.uint8), int(offsets[-1]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.sg_unitigs(arcs, reads, offsets)
        ran = ctx.profile_get()
        assert {"k_ut_links", "k_ut_mates", "k_ut_init", "k_ut_round", "k_ut_cut", "k_ut_tails", "k_ut_write"} <= set(ran)
        assert ran["k_ut_round"][0] == 2 * 6 and ran["k_ut_init"][0] == 2  # ceil(log2(54)) rounds, twice: nothing depends on the unitigs
        ctx.profile_reset()
        ctx.sg_unitig_seqs(want[0], want[1], bases, offsets)
        assert {"k_ut_seq_lens", "k_ut_seq_check", "k_ut_seq_offs", "k_ut_seq_ends", "k_ut_seq_copy"} <= set(ctx.profile_get())
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

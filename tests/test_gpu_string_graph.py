"""The string graph on the device (kmu_sg_classify, kmu_sg_graph and the wrappers above them) against the references of
tests/test_string_graph_abi.py: every output whole array against whole array, byte for byte, on host arrays and on resident tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import (ALN, ARC, CHAIN, READ, Refused, layout_records, offsets_of, out_degrees, params, planted_pile,  # noqa: E402
                                   planted_random, planted_reference, planted_tiling, records, reduced_records, reference_classify,
                                   reference_graph)

pytestmark = pytest.mark.gpu
T = A.SG_TILE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def to_device(chains, aln, offsets):
    import torch
    return (torch.from_numpy(np.ascontiguousarray(chains).view(np.int32).reshape(-1, 10)).cuda(),
            None if aln is None else torch.from_numpy(np.ascontiguousarray(aln).view(np.int32).reshape(-1, 4)).cuda(),
            torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda())


def to_host(arcs, arc_off, classes, reads):
    return (arcs.cpu().numpy().reshape(-1).view(ARC), arc_off.cpu().numpy().view(np.uint64), classes.cpu().numpy(),
            reads.cpu().numpy().reshape(-1).view(READ))


def same(got, want, what):
    for name, g, w in zip(("arcs", "arc_offsets", "classes", "reads"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g[:8], w[:8])


def check(ctx, chains, aln, offsets, p, want=None, what=""):
    """both modes of sg_graph and of sg_classify against the reference; returns the reference's outputs"""
    want = want if want is not None else reference_graph(chains, aln, offsets, **p)
    same(ctx.sg_graph(chains, aln, offsets, **p), want, what + " host")
    d = to_device(chains, aln, offsets)
    same(to_host(*ctx.sg_graph(*d, **p)), want, what + " device")
    bare = want[3].copy()
    bare["out_fwd"] = bare["out_rev"] = 0
    classes, reads = ctx.sg_classify(chains, aln, offsets, **p)
    assert classes.tobytes() == want[2].tobytes() and reads.tobytes() == bare.tobytes(), what + " classify host"
    classes, reads = ctx.sg_classify(*d, **p)
    assert classes.cpu().numpy().tobytes() == want[2].tobytes() and reads.cpu().numpy().tobytes() == bare.tobytes(), what + " classify device"
    return want


# ---- hand cases ----------------------------------------------------------------------------------------------------------------
def test_hand_cases(ctx):
    # each of the six classes, with alignment records (see tests/test_string_graph_abi.py for the arithmetic)
    off = offsets_of([1000, 1000, 1000, 300])
    aln = np.zeros(7, ALN)
    aln["flags"], aln["matches"], aln["edit"] = A.ALN_DONE, 900, 100
    aln[2] = (0xFFFFFFFF, 0, 2000, 0)
    chains = records([(1, 0, 0, 600, 1000, 0, 400), (0, 1, 0, 960, 1000, 0, 40), (0, 1, 0, 600, 1000, 0, 400), (0, 1, 0, 300, 700, 300, 700),
                      (0, 3, 0, 200, 500, 0, 300), (3, 0, 0, 0, 300, 200, 500), (0, 1, 0, 600, 1000, 0, 400)])
    want = check(ctx, chains, aln, off, params(min_identity_permille=900), what="classes")
    assert want[2].tolist() == [A.SG_SKIP, A.SG_SHORT, A.SG_LOWID, A.SG_INTERNAL, A.SG_B_CONTAINED, A.SG_SKIP, A.SG_DOVETAIL] and len(want[0]) == 2
    aln[6] = (101, 900, 9, A.ALN_DONE)  # one edit under the identity bound
    assert check(ctx, chains, aln, off, params(min_identity_permille=900))[2][6] == A.SG_LOWID
    # the four strand / side combinations in one batch of four pairs
    off = offsets_of([1000, 800] * 4)
    chains = records([(0, 1, 0, 700, 1000, 0, 300), (2, 3, 0, 0, 250, 550, 800), (4, 5, 1, 700, 1000, 500, 800), (6, 7, 1, 0, 250, 0, 250)])
    want = check(ctx, chains, None, off, params(), what="dovetails")
    assert [tuple(x)[:5] for x in want[0].tolist()] == [(0, 2, 500, 300, 0), (3, 1, 700, 300, 0), (5, 7, 550, 250, 1), (6, 4, 750, 250, 1),
                                                        (8, 11, 500, 300, 2), (10, 9, 700, 300, 2), (13, 14, 550, 250, 3), (15, 12, 750, 250, 3)]
    # containment: both ties, and the chain 0 c 1 c 2 with a dovetail 2 - 3
    check(ctx, records([(0, 1, 0, 0, 500, 0, 500)]), None, offsets_of([500, 500]), params(), what="tie")
    check(ctx, records([(0, 1, 0, 10, 490, 10, 510)]), None, offsets_of([500, 520]), params(), what="tie a")
    check(ctx, records([(0, 1, 0, 10, 510, 10, 490)]), None, offsets_of([520, 500]), params(), what="tie b")
    off = offsets_of([200, 400, 1000, 1000])
    chains = records([(0, 1, 0, 0, 200, 100, 300), (1, 2, 0, 0, 400, 300, 700), (2, 3, 0, 600, 1000, 0, 400), (1, 3, 0, 300, 400, 0, 100)])
    assert check(ctx, chains, None, off, params(), what="chain")[3]["flags"].tolist() == [1, 1, 0, 0]
    # the hang bounds at equality and one above
    off = offsets_of([2000, 2000])
    for b0, kw, cls in ((100, dict(max_hang=100, int_permille=1000), A.SG_DOVETAIL), (101, dict(max_hang=100, int_permille=1000), A.SG_INTERNAL),
                        (150, dict(int_permille=250), A.SG_DOVETAIL), (151, dict(int_permille=250), A.SG_INTERNAL),
                        (0, dict(max_hang=0, int_permille=0), A.SG_DOVETAIL)):
        assert check(ctx, records([(0, 1, 0, 1400, 2000, b0, b0 + 500)]), None, off, params(**kw))[2].tolist() == [cls]


def line_record(a, b, dist):
    """reads of 1 000 bases on one strand, b `dist` to the right of a: the arcs a+ -> b+ and b- -> a- of length dist"""
    return (a, b, 0, dist, 1000, 0, 1000 - dist)


def test_the_rule_at_its_bounds(ctx):
    off = offsets_of([1000] * 5)
    flags = {}
    # v = 1, w = 2, x = 3: f = 100, g = 200, and v -> x claims len_vx.  w -> y = 50 (y = 4) keeps g from being first(w); z = 0, 50 to the
    # left of w, does the same for the mates, where x- -> w- (200) and w- -> v- (100) meet the same bound
    for len_vx, fuzz in ((300, 0), (299, 0), (290, 10), (289, 10)):
        chains = records([line_record(1, 2, 100), line_record(1, 3, len_vx), line_record(2, 3, 200), line_record(2, 4, 50), line_record(0, 2, 50)])
        arcs = check(ctx, chains, None, off, params(fuzz=fuzz), what="rule %d %d" % (len_vx, fuzz))[0]
        flags[len_vx, fuzz] = int(arcs["flags"][arcs["rec"] == 1][0])
    assert flags == {(300, 0): 1, (299, 0): 0, (290, 10): 1, (289, 10): 0}
    # first(w) alone: without w -> y the arc g is the smallest of w and marks whatever the lengths
    chains = records([line_record(0, 1, 100), line_record(0, 2, 120), line_record(1, 2, 500)])
    assert reduced_records(check(ctx, chains, None, off, params(), what="first")[0]) == {1}


# ---- planted layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [0, 3])
def test_planted_tiling(ctx, jitter):
    chains, offsets, _, p = planted_tiling(jitter)
    arcs = check(ctx, chains, None, offsets, p, planted_reference("tiling", jitter), "tiling")[0]
    assert len(arcs) == 150 and len(reduced_records(arcs)) == 49


def test_planted_random_layout(ctx):
    chains, offsets, _, p, _, _ = planted_random()
    reads = check(ctx, chains, None, offsets, p, planted_reference("random"), "random")[3]
    assert out_degrees(reads).max() == 1 and reads["flags"].any()


@pytest.mark.parametrize("n", [63, 64, 65, 66, 130])
def test_planted_piles(ctx, n):
    chains, offsets, _, p = planted_pile(n)
    arcs, arc_off, _, _ = check(ctx, chains, None, offsets, p, planted_reference("pile", n), "pile")
    assert len(arcs) == n * (n - 1) and int((arc_off[1:] - arc_off[:-1]).max()) == n - 1


# ---- sizes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1])
def test_record_counts(ctx, n):
    chains, offsets, _ = layout_records(np.arange(80) * 2, np.full(80, 400), seed=21)  # 3 160 records, shuffled
    assert len(chains) >= 3 * T + 1
    arcs = check(ctx, chains[:n], None, offsets, params(), what="n = %d" % n)[0]
    assert len(arcs) == 2 * n


def test_no_dovetail_and_all_contained(ctx):
    off = offsets_of([1000, 1000, 500])
    chains = records([(0, 1, 0, 300, 700, 300, 700), (0, 2, 0, 990, 1000, 0, 10), (1, 0, 0, 600, 1000, 0, 400), (1, 2, 1, 100, 600, 0, 500)])
    arcs, arc_off, classes, reads = check(ctx, chains, None, off, params(), what="nothing")
    assert len(arcs) == 0 and not arc_off.any() and A.SG_DOVETAIL not in classes.tolist()
    # two records of one pair that disagree: each read is contained by one of them; the dovetail between them makes no arcs
    off = offsets_of([500, 520])
    chains = records([(0, 1, 0, 10, 490, 10, 510), (0, 1, 0, 5, 495, 0, 520), (0, 1, 0, 300, 500, 0, 200)])
    arcs, arc_off, classes, reads = check(ctx, chains, None, off, params(), what="contained")
    assert classes.tolist() == [A.SG_A_CONTAINED, A.SG_B_CONTAINED, A.SG_DOVETAIL] and reads["flags"].tolist() == [1, 1] and len(arcs) == 0


def spread(chains, offsets, gap, seed):
    """the same records with `gap` isolated reads, some of them empty, between any two reads"""
    rng = np.random.default_rng(seed)
    n = len(offsets) - 1
    lengths = rng.integers(0, 3, n * (gap + 1)) * rng.integers(1, 900, n * (gap + 1))
    lengths[::gap + 1] = np.diff(offsets.astype(np.int64))
    out = chains.copy()
    out["read_a"], out["read_b"] = chains["read_a"] * (gap + 1), chains["read_b"] * (gap + 1)
    return out, offsets_of(lengths)


def test_duplicates_empty_reads_and_isolated_reads(ctx):
    chains, offsets, _, p = planted_tiling(3)
    doubled = np.concatenate([chains, chains[::3], chains[:5]])
    arcs = check(ctx, doubled, None, offsets, p, what="duplicates")[0]
    assert len(arcs) == 2 * len(doubled) and len(set(zip(arcs["from"].tolist(), arcs["to"].tolist()))) == 150
    far, far_off = spread(chains, offsets, 75, seed=3)  # 2 052 reads, 2 025 of them isolated
    assert len(far_off) - 1 > 2000 and (np.diff(far_off.astype(np.int64)) == 0).sum() > 100
    got = check(ctx, far, None, far_off, p, what="isolated")
    assert len(got[0]) == 150 and len(reduced_records(got[0])) == 49
    # records on empty reads: every coordinate is 0; with min_overlap 0 they are containments at equal length
    empty = records([(0, 1, 0, 0, 0, 0, 0), (1, 2, 1, 0, 0, 0, 0)])
    got = check(ctx, empty, None, offsets_of([0, 0, 0]), params(min_overlap=0), what="empty")
    assert got[2].tolist() == [A.SG_B_CONTAINED, A.SG_B_CONTAINED]
    assert check(ctx, empty, None, offsets_of([0, 0, 0]), params())[2].tolist() == [A.SG_SHORT, A.SG_SHORT]


def test_the_order_of_the_records_changes_nothing(ctx):
    chains, offsets, _, p, _, _ = planted_random()
    order = np.random.default_rng(9).permutation(len(chains))
    a = ctx.sg_graph(chains, None, offsets, **p)
    b = ctx.sg_graph(chains[order], None, offsets, **p)
    assert a[2][order].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes() and a[1].tobytes() == b[1].tobytes()
    # no pair has two records here, so (from, to) alone orders the arcs: every field but rec is the same bytes, rec names the same record
    named = b[0].copy()
    named["rec"] = order[b[0]["rec"]]
    assert a[0].tobytes() == named.tobytes()


# ---- counting, capacity, NULL outputs and the refusals: the C entry points as they are -------------------------------------------
class Raw:
    """the arrays of one raw call, prefilled so that an output that was written shows"""

    def __init__(self, chains, offsets, p=None, cap=None, aln=None):
        self.chains, self.off, self.aln = np.ascontiguousarray(chains), np.ascontiguousarray(offsets), aln
        self.n, self.n_reads = len(chains), len(offsets) - 1
        self.p = A.SgParams(*[(p or params())[k] for k in ("min_overlap", "max_hang", "int_permille", "min_identity_permille", "fuzz")], 0)
        self.cap = 2 * self.n if cap is None else cap
        self.cls = np.full(max(self.n, 1), 0xAB, np.uint8)
        self.reads = np.full(max(self.n_reads, 1) * 4, 0xABABABAB, np.uint32)
        self.arcs = np.full(max(self.cap, 1) * 8, 0xABABABAB, np.uint32)
        self.arc_off = np.full(2 * self.n_reads + 1, 0xABABABABABABABAB, np.uint64)
        self.total = C.c_uint64(12345)

    def untouched(self):
        return (self.cls == 0xAB).all() and (self.reads == 0xABABABAB).all() and (self.arcs == 0xABABABAB).all() and (
            self.arc_off == 0xABABABABABABABAB).all()

    def head(self, ctx, mem=A.MEM_HOST, n=None, n_reads=None):
        return (ctx.h, self.chains.ctypes.data, None if self.aln is None else self.aln.ctypes.data, self.n if n is None else n, self.off.ctypes.data,
                self.n_reads if n_reads is None else n_reads, C.byref(self.p), mem)

    def graph(self, ctx, cls=True, reads=True, arcs=True, arc_off=True, **kw):
        return ctx.L.kmu_sg_graph(*self.head(ctx, **kw), self.cls.ctypes.data if cls else None, self.reads.ctypes.data if reads else None,
                                  self.arcs.ctypes.data if arcs else None, self.cap, self.arc_off.ctypes.data if arc_off else None,
                                  C.byref(self.total))

    def classify(self, ctx, **kw):
        return ctx.L.kmu_sg_classify(*self.head(ctx, **kw), self.cls.ctypes.data, self.reads.ctypes.data)


def test_count_capacity_and_null_outputs(ctx):
    chains, offsets, _, p = planted_tiling(0)
    want = planted_reference("tiling", 0)
    r = Raw(chains, offsets, p)
    assert r.graph(ctx, arcs=False) == 0 and r.total.value == 150 and r.untouched()            # count only: nothing but the total
    assert r.graph(ctx, cls=False, reads=False, arcs=False, arc_off=False) == 0 and r.total.value == 150
    r = Raw(chains, offsets, p, cap=149)
    assert r.graph(ctx) == A.E_BAD_ARG and r.total.value == 150 and r.untouched()              # one too small
    r = Raw(chains, offsets, p, cap=150)
    assert r.graph(ctx, cls=False, reads=False, arc_off=False) == 0 and r.arcs.tobytes() == want[0].tobytes()
    assert (r.cls == 0xAB).all() and (r.reads == 0xABABABAB).all()
    r = Raw(chains, offsets, p)                                                                 # 2 * DOVETAIL records is enough
    assert r.graph(ctx) == 0 and r.arcs[:150 * 8].tobytes() == want[0].tobytes() and (r.arcs[150 * 8:] == 0xABABABAB).all()
    assert r.cls.tobytes() == want[2].tobytes() and r.reads.tobytes() == want[3].tobytes() and r.arc_off.tobytes() == want[1].tobytes()
    # no records: no arcs, every summary zero, every offset 0
    r = Raw(chains[:0], offsets, p, cap=0)
    assert r.graph(ctx) == 0 and r.total.value == 0 and not r.reads.any() and not r.arc_off.any()
    assert r.classify(ctx) == 0 and not r.reads.any()


FAULTS = {
    "read_a": dict(read_a=27), "read_b": dict(read_b=0xFFFFFFFF), "strand": dict(strand=2), "a_order": dict(a_start=301, a_end=300),
    "b_order": dict(b_start=5, b_end=4), "a_end": dict(a_end=401), "b_end": dict(b_end=401),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
@pytest.mark.parametrize("at", [0, 40])
def test_device_found_refusals(ctx, fault, at):
    chains, offsets, _, p = planted_tiling(0)
    bad = chains.copy()
    if at == 40:  # in a record the graph would skip anyway: the faults are those of every record
        bad["read_a"][at], bad["read_b"][at] = bad["read_b"][at], bad["read_a"][at]
    for k, v in FAULTS[fault].items():
        bad[k][at] = v
    with pytest.raises(Refused):
        reference_classify(bad, None, offsets, **p)
    r = Raw(bad, offsets, p)
    assert r.graph(ctx) == A.E_UNSUPPORTED and r.untouched() and r.total.value == 12345
    assert r.classify(ctx) == A.E_UNSUPPORTED and r.untouched()
    d = to_device(bad, None, offsets)
    with pytest.raises(lib.KmuError) as e:
        ctx.sg_graph(*d, **p)
    assert e.value.code == A.E_UNSUPPORTED
    check(ctx, chains, None, offsets, p, planted_reference("tiling", 0), "after a refusal")


def test_bad_arguments(ctx):
    chains, offsets, _, p = planted_tiling(0)
    for kw in (dict(int_permille=1001), dict(min_identity_permille=1001)):
        r = Raw(chains, offsets, params(**kw))
        assert r.graph(ctx) == A.E_BAD_ARG and r.classify(ctx) == A.E_BAD_ARG and r.untouched()
    r = Raw(chains, offsets, p)
    r.p.flags = 1
    assert r.graph(ctx) == A.E_BAD_ARG and r.classify(ctx) == A.E_BAD_ARG and r.untouched()
    r = Raw(chains, offsets, p)
    assert r.graph(ctx, mem=2) == A.E_BAD_ARG and r.classify(ctx, mem=-1) == A.E_BAD_ARG
    assert r.graph(ctx, n=1 << 31) == A.E_UNSUPPORTED and r.classify(ctx, n_reads=1 << 31) == A.E_UNSUPPORTED
    assert r.graph(ctx, n_reads=0) == A.E_BAD_ARG and r.untouched()
    L = ctx.L
    head = r.head(ctx)
    assert L.kmu_sg_graph(*head, None, None, None, 0, None, None) == A.E_BAD_ARG                       # n_out
    assert L.kmu_sg_classify(*head, None, r.reads.ctypes.data) == A.E_BAD_ARG
    assert L.kmu_sg_classify(*head, r.cls.ctypes.data, None) == A.E_BAD_ARG
    assert L.kmu_sg_graph(ctx.h, None, None, 75, *head[4:], None, None, None, 0, None, C.byref(r.total)) == A.E_BAD_ARG   # chains
    assert L.kmu_sg_graph(*head[:4], None, *head[5:], None, None, None, 0, None, C.byref(r.total)) == A.E_BAD_ARG       # offsets
    assert L.kmu_sg_graph(*head[:6], None, head[7], None, None, None, 0, None, C.byref(r.total)) == A.E_BAD_ARG         # p
    assert r.untouched()


def test_alignment_records_that_pass_everything(ctx):
    chains, offsets, _, p = planted_tiling(3)
    aln = np.zeros(len(chains), ALN)
    aln["flags"], aln["matches"], aln["edit"] = A.ALN_DONE | A.ALN_EXACT, 300, 40
    with_aln = ctx.sg_graph(chains, aln, offsets, **p)
    same(with_aln, ctx.sg_graph(chains, None, offsets, **p), "aln")
    same(with_aln, planted_reference("tiling", 3), "aln")


# ---- the wrappers --------------------------------------------------------------------------------------------------------------
def test_unitig_labels_and_gfa(ctx):
    chains, offsets, _, p = planted_tiling(0)
    want = planted_reference("tiling", 0)
    arcs, _, _, reads = minimizer.overlap_graph(ctx, chains, None, offsets, **p)
    labels = minimizer.unitig_labels(ctx, arcs, 27)
    assert labels.dtype == np.uint32 and labels.tolist() == [0] * 27
    d_arcs = minimizer.overlap_graph(ctx, *to_device(chains, None, offsets), **p)[0]
    assert minimizer.unitig_labels(ctx, d_arcs, 27).cpu().tolist() == [0] * 27
    names = ["read%d" % i for i in range(27)]
    lines = ["S\tread%d\t*\tLN:i:400" % i for i in range(27)]
    lines += ["L\tread%d\t%s\tread%d\t%s\t%dM" % (x["from"] >> 1, "+-"[x["from"] & 1], x["to"] >> 1, "+-"[x["to"] & 1], x["ovl"])
              for x in want[0] if not x["flags"]]
    assert minimizer.gfa_lines(arcs, names, offsets, reads=reads) == lines and len(lines) == 27 + 52
    assert len(minimizer.gfa_lines(arcs, names, offsets, reduced=True)) == 27 + 150
    # contained reads have no segment line
    chains, offsets, _, p, _, _ = planted_random()
    arcs, _, _, reads = minimizer.overlap_graph(ctx, chains, None, offsets, **p)
    got = minimizer.gfa_lines(arcs, ["r%d" % i for i in range(120)], offsets, reads=reads)
    assert sum(1 for x in got if x[0] == "S") == 120 - int((reads["flags"] & 1).sum())


def test_read_graph_end_to_end(ctx):
    import torch
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 6000).astype(np.uint8)
    k, w, n = 15, 5, 60
    codes = np.lib.stride_tricks.sliding_window_view(genome, k).astype(np.uint64) @ (4 ** np.arange(k, dtype=np.uint64))
    rc = np.lib.stride_tricks.sliding_window_view((3 - genome)[::-1], k).astype(np.uint64) @ (4 ** np.arange(k, dtype=np.uint64))
    assert len(set(codes.tolist()) | set(rc.tolist())) == 2 * len(codes)  # no repeat at k = 15, on either strand
    starts = np.round(np.arange(n) * (5400 / (n - 1))).astype(np.int64)
    order = rng.permutation(n)
    lut, parts = np.frombuffer(b"ACGT", np.uint8), []
    for i in order:
        piece = genome[starts[i]:starts[i] + 600]
        parts.append(lut[(3 - piece)[::-1]] if rng.integers(0, 2) else lut[piece])
    bases, offsets = np.concatenate(parts), offsets_of([600] * n)
    p = params(min_overlap=100, fuzz=10)
    d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()
    got = to_host(*minimizer.read_graph(ctx, d_bases, d_off, k, w, **p))
    # every stage's own output goes into the reference
    d_chains, d_aln = minimizer.read_alignments(ctx, d_bases, d_off, k, w)
    chains, aln = d_chains.cpu().numpy().reshape(-1).view(CHAIN), d_aln.cpu().numpy().reshape(-1).view(ALN)
    assert len(chains) >= n - 1
    same(got, reference_graph(chains, aln, offsets, **p), "read_graph")
    assert not got[3]["flags"].any() and sorted(out_degrees(got[3]).tolist()) == [0, 0] + [1] * (2 * n - 2)
    labels = minimizer.unitig_labels(ctx, minimizer.read_graph(ctx, d_bases, d_off, k, w, **p)[0], n)
    assert labels.cpu().tolist() == [0] * n
    # the survivors join neighbours of the tiling
    alive = got[0][got[0]["flags"] == 0]  # (read r is piece order[r] of the tiling)
    assert all(abs(int(order[x["from"] >> 1]) - int(order[x["to"] >> 1])) == 1 for x in alive)


def test_the_kernels_that_ran(ctx):
    chains, offsets, _, p = planted_tiling(0)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.sg_graph(chains, None, offsets, **p)
        ran = set(ctx.profile_get())
        assert {"k_sg_classify", "k_sg_arcs_count", "k_sg_arcs_write", "k_sort_hist", "k_sort_scatter", "k_sg_fill", "k_sg_heads", "k_sg_reduce",
                "k_sg_finish", "k_sg_unique"} <= ran
        ctx.profile_reset()
        ctx.sg_classify(chains, None, offsets, **p)
        assert set(ctx.profile_get()) == {"k_sg_classify"}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

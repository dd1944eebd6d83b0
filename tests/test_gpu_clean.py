"""String graph cleaning on the device (kmu_sg_clean and the wrappers above it) against reference_clean of tests/test_clean_abi.py:
arcs, reads and stats whole array against whole array, byte for byte, on host arrays and on resident tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import ARC, READ, Refused, offsets_of, params, planted_reference, records  # noqa: E402
from test_unitigs_abi import PLACE, STEP, UNITIG, hostile_graph, reference_unitigs  # noqa: E402
from test_clean_abi import (CASES, LIMITS, STATS, cleaned_case, faulty_graphs, planted, planted_case, reference_clean,  # noqa: E402
                            removed_reads)

pytestmark = pytest.mark.gpu
COPIES = 1000  # of the mix in one call: beyond one pass of the grid


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


def host(x, dtype):
    return x.cpu().numpy().reshape(-1).view(dtype)


def same(got, want, what):
    for name, g, w in zip(("arcs", "reads"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (what, name, g[:8], w[:8])
    assert got[2] == want[2], (what, got[2], want[2])


def check(ctx, arcs, reads, n_reads, T, B, want=None, what=""):
    """both modes of sg_clean against the reference; returns the reference's outputs"""
    want = want if want is not None else reference_clean(arcs, n_reads, T, B, reads)
    same(ctx.sg_clean(arcs, reads, n_reads, T, B), want, what + " host")
    got = ctx.sg_clean(dev(arcs, 8), dev(reads, 4), n_reads, T, B)
    assert got[0].is_cuda and got[1].is_cuda
    same((host(got[0], ARC), host(got[1], READ), got[2]), want, what + " device")
    return want


@pytest.mark.parametrize("T,B", LIMITS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_planted_cases(ctx, name, T, B):
    arcs, n_reads, _ = planted_case(name)
    check(ctx, arcs, None, n_reads, T, B, cleaned_case(name, T, B), name)


@pytest.mark.parametrize("n,T", [(63, 64), (64, 64), (65, 64), (3, 3), (4, 3)])
def test_tip_walk_limits(ctx, n, T):
    arcs, n_reads, _ = planted(n + 70, [(n, n + 2, False)], [], seed=n)
    want = check(ctx, arcs, None, n_reads, T, 0, what="tip of %d" % n)
    assert want[2]["n_tip_reads"] == (n if n <= T else 0)


@pytest.mark.parametrize("k,B,m", [(64, 64, 2), (65, 64, 1), (2, 2, 1), (3, 2, 1)])
def test_branch_walk_limits(ctx, k, B, m):
    arcs, n_reads, _ = planted(12, [], [(k, m, 4)], seed=k)
    want = check(ctx, arcs, None, n_reads, 0, B, what="branch of %d" % k)
    assert want[2]["n_bubbles"] == (1 if k <= B else 0)


def test_many_copies_in_one_call_and_a_second_round(ctx):
    arcs, n_reads, _ = planted_case("mix", 3, COPIES)
    assert n_reads == 107 * COPIES and len(arcs) == 222 * COPIES
    want = cleaned_case("mix", 4, 8, 3, COPIES)
    assert want[2]["n_tips"] == 8 * COPIES and want[2]["n_bubbles"] == 5 * COPIES and want[2]["n_spared"] == COPIES
    check(ctx, arcs, None, n_reads, 4, 8, want, "copies")
    # the output of one call is the input of the next: the tip of 5 reads is a tip of 5 still, nothing else is left to remove
    again = check(ctx, want[0], want[1], n_reads, 4, 8, what="second round")
    assert again[2]["n_tip_reads"] == 0 and again[2]["n_arcs_left"] == want[2]["n_arcs_left"]
    got = minimizer.clean_graph(ctx, arcs, None, n_reads, 4, 8, rounds=3)
    assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
    assert got[2] == {k: again[2][k] if k == "n_arcs_left" else want[2][k] + again[2][k] for k in STATS}


@pytest.mark.parametrize("name,arg", [("tiling", 0), ("tiling", 3), ("random", None), ("pile", 65)])
def test_planted_layouts_come_back_as_they_are(ctx, name, arg):
    arcs, _, _, reads = planted_reference(name, arg)
    for T, B in ((4, 8), (64, 64)):
        want = check(ctx, arcs, reads, len(reads), T, B, what=name)
        assert want[0].tobytes() == arcs.tobytes() and want[1].tobytes() == reads.tobytes()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_hostile_graphs_come_back_as_they_are(ctx, seed):
    arcs, reads, _, _ = hostile_graph(seed)
    want = check(ctx, arcs, reads, len(reads), 4, 8, what="hostile")
    assert want[0].tobytes() == arcs.tobytes() and want[1].tobytes() == reads.tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class Raw:
    """the entry point itself on prefilled outputs, host arrays or resident tensors"""

    def __init__(self, arcs, reads, n_reads, device=False):
        self.device, self.n_reads = device, n_reads
        fill = lambda dtype, n: np.frombuffer(bytes([0xAB]) * (dtype.itemsize * n), dtype).copy()  # noqa: E731
        self.outs = [fill(ARC, max(len(arcs), 1)), fill(READ, max(n_reads, 1))]
        self.want = [x.tobytes() for x in self.outs]
        self.ins = [np.ascontiguousarray(arcs), reads]
        if device:
            self.ins = [dev(self.ins[0], 8), dev(reads, 4)]
            self.outs = [dev(self.outs[0], 8), dev(self.outs[1], 4)]
        self.stats = A.SgCleanStats(*([12345] * 8))

    def call(self, c, T=4, B=8, **kw):
        p = lambda x: lib._ptr(x)[0]  # noqa: E731
        args = dict(ctx=c.h, arcs=p(self.ins[0]), n_arcs=int(self.ins[0].shape[0]), reads=p(self.ins[1]), n_reads=self.n_reads,
                    p=C.byref(A.SgCleanParams(T, B, 0, 0)), mem=A.MEM_DEVICE if self.device else A.MEM_HOST, arcs_out=p(self.outs[0]),
                    reads_out=p(self.outs[1]), stats=C.byref(self.stats))
        args.update(kw)
        return c.L.kmu_sg_clean(*args.values())

    def untouched(self):
        got = [host(x, np.uint8).tobytes() if self.device else x.tobytes() for x in self.outs]
        return got == self.want and [getattr(self.stats, k) for k in STATS] == [12345] * 8


@pytest.mark.parametrize("fault", sorted(faulty_graphs()))
def test_device_found_refusals(ctx, fault):
    arcs, reads, n_reads = faulty_graphs()[fault]
    with pytest.raises(Refused):
        reference_clean(arcs, n_reads, 4, 8, reads)
    for device in (False, True):
        r = Raw(arcs, reads, n_reads, device)
        assert r.call(ctx) == A.E_UNSUPPORTED and r.untouched(), (fault, device)
    with pytest.raises(lib.KmuError) as e:
        ctx.sg_clean(arcs, reads, n_reads)
    assert e.value.code == A.E_UNSUPPORTED
    name = "tips in"  # a good call after a refused one
    check(ctx, planted_case(name)[0], None, planted_case(name)[1], 4, 8, cleaned_case(name, 4, 8), "after a refusal")


def test_a_fault_among_many_arcs(ctx):
    """the same faults far from the first workgroup"""
    arcs, n_reads, _ = planted_case("mix", 3, COPIES)
    for fault in ("unsorted", "out of range", "no mate"):
        bad = arcs.copy()
        i = len(bad) - 5000
        if fault == "unsorted":
            bad["from"][i] = 0
        elif fault == "out of range":
            bad["to"][i] = 2 * n_reads
        else:
            bad["rec"][i] ^= 1 << 20
        for device in (False, True):
            r = Raw(bad, None, n_reads, device)
            assert r.call(ctx) == A.E_UNSUPPORTED and r.untouched(), (fault, device)


def test_bad_arguments(ctx):
    arcs, n_reads, _ = planted_case("tips in")
    r = Raw(arcs, None, n_reads)
    null = C.POINTER(A.SgCleanParams)()
    for kw in (dict(p=null), dict(stats=None), dict(arcs=None), dict(arcs_out=None), dict(mem=2), dict(mem=-1), dict(T=65), dict(B=65),
               dict(p=C.byref(A.SgCleanParams(4, 8, 1, 0))), dict(p=C.byref(A.SgCleanParams(4, 8, 0, 1))), dict(n_reads=0),
               dict(arcs_out=lib._ptr(arcs)[0]), dict(ctx=None)):
        assert r.call(ctx, **kw) == A.E_BAD_ARG and r.untouched(), kw
    assert r.call(ctx, n_reads=1 << 31) == A.E_UNSUPPORTED and r.untouched()
    assert r.call(ctx, n_arcs=1 << 32) == A.E_UNSUPPORTED and r.untouched()
    # the optional ones may be null
    assert r.call(ctx, reads_out=None) == A.OK and r.outs[0].tobytes() == cleaned_case("tips in", 4, 8)[0].tobytes()
    assert r.outs[1].tobytes() == r.want[1] and r.stats.n_tips == 4


def test_no_arcs_and_one_read(ctx):
    reads = np.zeros(3, READ)
    reads["flags"], reads["n_records"], reads["out_fwd"] = [0, 1, 0], [4, 5, 6], [9, 9, 9]
    want = check(ctx, np.zeros(0, ARC), reads, 3, 4, 8, what="no arcs")
    assert want[1]["n_records"].tolist() == [4, 5, 6] and not want[1]["out_fwd"].any() and not any(want[2].values())
    check(ctx, np.zeros(0, ARC), None, 1, 4, 8, what="one read")
    r = Raw(np.zeros(0, ARC), None, 0)
    assert r.call(ctx, arcs=None, arcs_out=None, reads_out=None) == A.OK and [getattr(r.stats, k) for k in STATS] == [0] * 8


# ---- through the layout ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_through_the_layout(ctx, name):
    arcs, n_reads, groups = planted_case(name)
    want = cleaned_case(name, 4, 8)
    off = offsets_of(np.full(n_reads, 1000))
    arcs_out, reads_out, _ = ctx.sg_clean(arcs, None, n_reads, 4, 8)
    laid = minimizer.layout_reads(reads_out)
    wanted = reference_unitigs(want[0], minimizer.layout_reads(want[1]), off)
    for g, w in zip(ctx.sg_unitigs(arcs_out, laid, off), wanted):
        assert g.tobytes() == w.tobytes(), name
    d = ctx.sg_clean(dev(arcs, 8), None, n_reads, 4, 8)
    got = ctx.sg_unitigs(d[0], minimizer.layout_reads(d[1]), dev(off))
    for g, w, dtype in zip(got, wanted, (UNITIG, STEP, PLACE)):
        assert host(g, dtype).tobytes() == w.tobytes(), name
    if name in ("tips in", "tips out"):
        gone = sorted(set(sum(groups[0]["tips"][:4], [])))
        assert gone == sorted(removed_reads(want[1])) and (wanted[2]["unitig"][gone] == A.SG_NONE).all()


def test_a_line_of_six_reads_and_one_tip_read_from_records(ctx):
    """reads of 1 000 bases, each 400 to the right of the one before; read 6 lies where read 2 does but is given one record only, its
    overlap with read 3 (`rec(...)` rows of tests/test_string_graph_abi.py): a dead end of one read that enters read 3 beside the stem 0, 1, 2, which is spared as the longer one"""
    rows = [(i, i + 1, 0, 400, 1000, 0, 600) for i in range(5)] + [(3, 6, 0, 0, 600, 400, 1000)]
    chains, off = records(rows), offsets_of([1000] * 7)
    for device in (False, True):
        args = (dev(chains, 10), None, dev(off)) if device else (chains, None, off)
        arcs, _, _, reads = minimizer.overlap_graph(ctx, *args, **params())
        arcs, reads, stats = minimizer.clean_graph(ctx, arcs, reads, 7)
        assert (stats["n_tips"], stats["n_tip_reads"], stats["n_spared"], stats["n_arcs_tip"], stats["n_arcs_left"]) == (1, 1, 1, 2, 10)
        unitigs, path, place = minimizer.unitig_paths(ctx, arcs, minimizer.layout_reads(reads), args[2])
        if device:
            unitigs, path, place = host(unitigs, UNITIG), host(path, STEP), host(place, PLACE)
        assert unitigs.tolist() == [(0, 3000, 6, 0, 0, 0)] and path["read"].tolist() == [0, 1, 2, 3, 4, 5]
        assert place["unitig"].tolist() == [0] * 6 + [A.SG_NONE]


def test_read_unitigs_with_nothing_to_remove(ctx):
    """the batch of test_read_unitigs_end_to_end (tests/test_gpu_unitigs.py): one line, so the limits change no byte"""
    rng = np.random.default_rng(77)
    genome = rng.integers(0, 4, 6000).astype(np.uint8)
    k, w, n = 15, 5, 60
    starts = np.round(np.arange(n) * (5400 / (n - 1))).astype(np.int64)
    lut, parts = np.frombuffer(b"ACGT", np.uint8), []
    for i in rng.permutation(n):
        piece = genome[starts[i]:starts[i] + 600]
        parts.append(lut[(3 - piece)[::-1]] if rng.integers(0, 2) else lut[piece])
    bases, offsets = np.concatenate(parts), offsets_of([600] * n)
    p = params(min_overlap=100, fuzz=10)
    today = minimizer.read_unitigs(ctx, bases, offsets, k, w, **p)
    assert today[0].tolist() == [(0, 6000, n, 0, 0, 0)]
    for kw in (dict(max_tip_reads=0, max_bubble_reads=0), dict(max_tip_reads=4, max_bubble_reads=8), dict(max_tip_reads=4, max_bubble_reads=8, clean_rounds=3)):
        for g, t in zip(minimizer.read_unitigs(ctx, bases, offsets, k, w, **p, **kw), today):
            assert g.dtype == t.dtype and g.tobytes() == t.tobytes(), kw
    graph = minimizer.read_graph(ctx, bases, offsets, k, w, **p)
    for g, t in zip(minimizer.read_graph(ctx, bases, offsets, k, w, max_tip_reads=4, max_bubble_reads=8, **p), graph):
        assert g.tobytes() == t.tobytes()


def test_the_kernels_that_ran(ctx):
    arcs, n_reads, _ = planted_case("mix")
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.sg_clean(arcs, None, n_reads, 4, 8)
        ran = ctx.profile_get()
        names = {"k_cl_check", "k_cl_tips", "k_cl_spare", "k_cl_tipkill", "k_cl_flag_tip", "k_cl_bubbles", "k_cl_flag_bubble", "k_cl_unique",
                 "k_cl_reads"}
        assert names <= set(ran) and all(ran[k][0] == 1 for k in names)  # nine launches, whatever the graph
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

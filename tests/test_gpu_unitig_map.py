"""The unitig map on the device (kmu_sg_unitig_chains and Context.sg_unitig_chains) against reference_unitig_chains of
tests/test_unitig_map_abi.py: records, stats and n_out whole array against whole array, byte for byte, on host arrays and on resident
tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_string_graph_abi import CHAIN, Refused  # noqa: E402
from test_unitig_map_abi import STATS, Builder, faulty_cases, mix, planted_genome, reference_unitig_chains  # noqa: E402

pytestmark = pytest.mark.gpu
COPIES = 4000  # of the mix in one call: beyond one pass of the grid
FEW = 200      # copies for the faults far from the first workgroup
COLS = (8, 4, 4, 10, None, None)  # int32 columns of unitigs, path, place, chains; classes and offsets are plain numbers


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


def check(ctx, arrays, what=""):
    """both modes of sg_unitig_chains against the reference; returns the reference's outputs"""
    want = reference_unitig_chains(*arrays)
    got = ctx.sg_unitig_chains(*arrays)
    assert got[0].dtype == want[0].dtype and got[0].tobytes() == want[0].tobytes() and got[1] == want[1], (what, "host", got[1], want[1])
    got = ctx.sg_unitig_chains(*(dev(x, c) for x, c in zip(arrays, COLS)))
    assert got[0].is_cuda and host(got[0], CHAIN).tobytes() == want[0].tobytes() and got[1] == want[1], (what, "device", got[1], want[1])
    return want


def test_the_mix(ctx):
    """unitigs of 1, 2, 64 and 65 reads, reverse steps, a circle, a late long read, ties, both record sides, strands, a contained
    container and a start below 0 (the answers are written out in tests/test_unitig_map_abi.py)"""
    b, _ = mix()
    records, stats = check(ctx, b.arrays(), "mix")
    assert stats == dict(n_layout=143, n_contained=8, n_unplaced=2) and len(records) == 151


def test_without_records(ctx):
    b, _ = mix()
    unitigs, path, place, _, _, off = b.arrays()
    records, stats = check(ctx, (unitigs, path, place, None, None, off), "chains=None")
    assert stats["n_contained"] == 0 and len(records) == 143
    got = minimizer.unitig_read_chains(ctx, unitigs, path, place, None, None, off)
    assert got[0].tobytes() == records.tobytes() and got[1] == stats


def test_many_copies_in_one_call(ctx):
    """more reads than one pass of the grid holds lanes (8 workgroups of 256 on each of 256 CUs); the wanted records are those of
    one copy, shifted (tests/test_unitig_map_abi.py checks that against the reference on two copies)"""
    b, _ = mix()
    arrays = b.arrays(COPIES)
    assert len(arrays[2]) == len(b.lens) * COPIES > 256 * 8 * 256
    one, _ = reference_unitig_chains(*b.arrays())
    want, k = np.tile(one, COPIES), np.repeat(np.arange(COPIES), len(one))
    cont = want["score"] == 1
    want["read_a"] += (k * len(b.unitigs)).astype(np.uint32)
    want["read_b"] += (k * len(b.lens)).astype(np.uint32)
    want["n_seeds"][cont] += (k * len(b.chains)).astype(np.uint32)[cont]
    want["n_anchors"][cont] += (k * len(b.lens)).astype(np.uint32)[cont]
    stats = dict(n_layout=143 * COPIES, n_contained=8 * COPIES, n_unplaced=2 * COPIES)
    got = ctx.sg_unitig_chains(*arrays)
    assert got[0].tobytes() == want.tobytes() and got[1] == stats
    got = ctx.sg_unitig_chains(*(dev(x, c) for x, c in zip(arrays, COLS)))
    assert host(got[0], CHAIN).tobytes() == want.tobytes() and got[1] == stats


@pytest.mark.parametrize("circular", [False, True])
def test_planted_genome(ctx, circular):
    g = planted_genome(5, circular, rate=0.05)
    check(ctx, (g["unitigs"], g["path"], g["place"], g["chains"], g["classes"], g["offsets"]), "genome")


def test_one_read_and_no_unitig(ctx):
    b = Builder()
    b.read(100)
    _, stats = check(ctx, b.arrays(), "one read, nothing placed")
    assert stats == dict(n_layout=0, n_contained=0, n_unplaced=1)
    b = Builder()
    b.unitig([(100, 0, 100)])
    records, _ = check(ctx, b.arrays(), "one read on one unitig")
    assert records.tolist() == [(0, 0, 0, 0, A.SG_NONE, A.SG_NONE, 0, 100, 0, 100)]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
class Raw:
    """the entry point itself on prefilled outputs, host arrays or resident tensors"""

    def __init__(self, arrays, device=False):
        self.device, self.n_reads = device, len(arrays[5]) - 1
        self.out = np.frombuffer(bytes([0xAB]) * (CHAIN.itemsize * max(self.n_reads, 1)), CHAIN).copy()
        self.want = self.out.tobytes()
        self.ins = [None if x is None else np.ascontiguousarray(x) for x in arrays]
        if device:
            self.ins = [dev(x, c) for x, c in zip(self.ins, COLS)]
            self.out = dev(self.out, 10)
        self.stats, self.n_out = A.UmStats(12345, 12345, 12345), C.c_uint64(12345)

    def call(self, c, **kw):
        p = lambda x: lib._ptr(x)[0] if x is not None and int(x.shape[0]) else None  # noqa: E731
        unitigs, path, place, chains, classes, off = self.ins
        args = dict(ctx=c.h, unitigs=p(unitigs), n_unitigs=int(unitigs.shape[0]), path=p(path), n_steps=int(path.shape[0]), place=p(place),
                    chains=p(chains), classes=p(classes), n_chains=0 if chains is None else int(chains.shape[0]), off=p(off),
                    n_reads=self.n_reads, p=C.byref(A.UmParams(0, 0)), mem=A.MEM_DEVICE if self.device else A.MEM_HOST, out=p(self.out),
                    stats=C.byref(self.stats), n_out=C.byref(self.n_out))
        args.update(kw)
        return c.L.kmu_sg_unitig_chains(*args.values())

    def untouched(self):
        got = host(self.out, np.uint8).tobytes() if self.device else self.out.tobytes()
        return got == self.want and [getattr(self.stats, k) for k in STATS] == [12345] * 3 and self.n_out.value == 12345


@pytest.mark.parametrize("fault", sorted(faulty_cases()))
def test_device_found_refusals(ctx, fault):
    arrays = faulty_cases()[fault]
    with pytest.raises(Refused):
        reference_unitig_chains(*arrays)
    for device in (False, True):
        r = Raw(arrays, device)
        assert r.call(ctx) == A.E_UNSUPPORTED and r.untouched(), (fault, device)
    with pytest.raises(lib.KmuError) as e:
        ctx.sg_unitig_chains(*arrays)
    assert e.value.code == A.E_UNSUPPORTED
    check(ctx, mix()[0].arrays(), "after a refusal")  # a good call after a refused one


def test_a_fault_among_many_records(ctx):
    """the same faults far from the first workgroup"""
    b, ids = mix()
    good = b.arrays(FEW)
    for which, field, index, value in ((1, "read", len(good[1]) - 5000, len(good[2])), (2, "rank", len(good[2]) - 30 * len(b.lens) + ids["line64"][3], 64),
                                       (3, "a_end", len(good[3]) - 25 * len(b.chains) + ids["tie_x"], 401), (0, "len", len(good[0]) - 9, 1 << 32)):
        arrays = [x.copy() for x in good]
        arrays[which][field][index] = value
        for device in (False, True):
            r = Raw(arrays, device)
            assert r.call(ctx) == A.E_UNSUPPORTED and r.untouched(), (which, field, device)


def test_bad_arguments(ctx):
    b, _ = mix()
    r = Raw(b.arrays())
    null = C.POINTER(A.UmParams)()
    for kw in (dict(p=null), dict(off=None), dict(stats=None), dict(n_out=None), dict(unitigs=None), dict(path=None), dict(place=None),
               dict(out=None), dict(chains=None), dict(classes=None), dict(mem=2), dict(mem=-1), dict(p=C.byref(A.UmParams(1, 0))),
               dict(p=C.byref(A.UmParams(0, 1))), dict(ctx=None)):
        assert r.call(ctx, **kw) == A.E_BAD_ARG and r.untouched(), kw
    assert r.call(ctx, n_reads=1 << 31) == A.E_UNSUPPORTED and r.untouched()
    assert r.call(ctx, n_chains=1 << 32) == A.E_UNSUPPORTED and r.untouched()
    # no reads: zero counts, whatever else is passed
    assert r.call(ctx, n_reads=0, place=None, out=None) == A.OK
    assert [getattr(r.stats, k) for k in STATS] == [0] * 3 and r.n_out.value == 0 and r.out.tobytes() == r.want
    # both record arrays may be null together
    r = Raw(b.arrays())
    assert r.call(ctx, chains=None, classes=None, n_chains=0) == A.OK and r.n_out.value == 143 and r.stats.n_unplaced == len(b.lens) - 143


def test_the_kernels_that_ran(ctx):
    b, _ = mix()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        ctx.sg_unitig_chains(*b.arrays())
        ran = ctx.profile_get()
        names = {"k_um_check", "k_um_cand", "k_um_flag", "k_um_write"}
        assert names <= set(ran) and all(ran[k][0] == 1 for k in names)  # four launches, whatever the data
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

"""-m gpu: kmu_pile_segments, kmu_extract_ranges and kmu_pile_consensus_pos against `reference_segments`, `reference_extract` and
`reference_cons_pos` (tests/test_trim_abi.py: the contracts of include/kmu.h in plain numpy).  Whole arrays are compared byte for
byte.  The segments depend on the table alone, so the edge cases synthesise tables and need no aligner; the planted truth goes
through Context.chain_cigar on hand-made chain records."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import batch, chain_recs  # noqa: E402
from test_consensus_abi import reference_consensus  # noqa: E402
from test_gpu_chain_align import ACGT, mutate  # noqa: E402
from test_gpu_pile_consensus import random_rows  # noqa: E402
from test_trim_abi import (EXT_TILE, SEG_TILE, deep_row_case, extract_cases, reference_cons_pos, reference_extract, reference_segments,  # noqa: E402
                           segment_cases, table)

pytestmark = pytest.mark.gpu
T = SEG_TILE
SEG, TRIM = np.dtype(A.PILE_SEG_DTYPE), np.dtype(A.READ_TRIM_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def words(x):
    """a record array, or a tensor that holds its bits, as a flat array of uint32 on the host"""
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint32)


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    got, want = words(got), words(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%s: %d words differ, the first at %d: got %s, want %s" % (what, bad.size, bad[0], got[bad[0]], want[bad[0]])


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


def check_segments(ctx, pile, offsets, rule, device=False):
    """host mode (and device mode) against the reference, with and without LONGEST; returns the reference's plain result"""
    import torch
    for longest in (False, True):
        want = reference_segments(pile, offsets, *rule, longest)
        got = ctx.pile_segments(pile, offsets, *rule, longest=longest)
        assert got[0].dtype == SEG and got[2].dtype == TRIM and got[1].dtype == np.uint64
        for g, w, what in zip(got, want, ("segs", "seg_offsets", "reads")):
            same(g, w, "%s %r longest=%d" % (what, rule, longest))
        if device:
            d = ctx.pile_segments(torch.from_numpy(pile.view(np.int32)).cuda(), offsets, *rule, longest=longest)
            assert all(x.is_cuda for x in d) and d[0].dtype == torch.int32 and d[1].dtype == torch.int64 and d[2].dtype == torch.int32
            for g, w, what in zip(d, want, ("segs", "seg_offsets", "reads")):
                same(g, w, "device %s %r longest=%d" % (what, rule, longest))
    return reference_segments(pile, offsets, *rule)


def random_table(rng, n, hi=6):
    """depths 0 .. 5 (hi - 1) per column, a third of the rows with ENDS 0, a few rows without any vote"""
    pile = rng.integers(0, hi, (n, 8)).astype(np.uint32)
    pile[rng.integers(0, 3, n) == 0, A.PILE_ENDS] = 0
    pile[rng.integers(0, 40, n) == 0, :5] = 0
    return pile


RULES = [(1, 0, 1), (10, 0, 1), (12, 8, 2), (13, 13, 5), (9, 11, 64)]


# ---- the hand cases of tests/test_trim_abi.py, on the device ------------------------------------------------------------------------
def test_hand_cases_on_the_device(ctx):
    def segments(pile, offsets, min_depth, min_span, min_len, longest):
        return ctx.pile_segments(pile, offsets, min_depth, min_span, min_len, longest=longest)
    segment_cases(segments)   # the flush join at min_span 0 and above, the clamp, LONGEST with ties, adjacent and empty reads, all bad
    deep_row_case(segments)   # the 2^32-depth row, min_depth 2^32 - 1
    extract_cases(ctx.extract_ranges)


# ---- the edges of the row tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, T - 1, T, T + 1, 5 * T + 3])
def test_row_tile_edges(ctx, n):
    """reads of n rows at the start of the batch, behind an empty read, and beginning on a tile boundary; host and device mode"""
    rng = np.random.default_rng(400 + n)
    lengths = [0, n, (T - n % T) % T, n, 3, 0]
    offsets = offsets_of(lengths)
    assert int(offsets[3]) % T == 0
    pile = random_table(rng, int(offsets[-1]))
    for k, rule in enumerate(RULES):
        check_segments(ctx, pile, offsets, rule, device=k == 2)
    same(ctx.pile_segments(pile[:n], offsets_of([n]), 10, 0, 1)[0], reference_segments(pile[:n], offsets_of([n]), 10, 0, 1)[0])


def test_runs_on_tile_edges(ctx):
    """a run that begins on a tile's first row and ends on its last, a run over more than three tiles, a run of one row at a tile's
    last position, and two all-good reads that meet on a tile boundary"""
    depths = np.full(8 * T, 5, np.int64)
    depths[[T - 1, 2 * T, 5 * T + 7, 6 * T - 2]] = 0
    offsets = offsets_of([6 * T, 2 * T])
    segs, seg_off, reads = check_segments(ctx, table(depths), offsets, (3, 0, 1), device=True)
    assert segs.tolist() == [(0, 0, T - 1, 0), (0, T, 2 * T, 1), (0, 2 * T + 1, 5 * T + 7, 2), (0, 5 * T + 8, 6 * T - 2, 3), (0, 6 * T - 1, 6 * T, 4), (1, 0, 2 * T, 0)]
    assert reads["cls"].tolist() == [A.TRIM_SPLIT, A.TRIM_WHOLE] and seg_off.tolist() == [0, 5, 6]
    # ... and linked by the spanning depth alone: ENDS equal to the depth on both sides of a tile boundary
    pile = table(depths, np.zeros(8 * T, np.int64))
    pile[[3 * T - 1, 3 * T], A.PILE_ENDS] = 5
    assert check_segments(ctx, pile, offsets, (3, 1, 1))[0].tolist()[2:4] == [(0, 2 * T + 1, 3 * T, 2), (0, 3 * T, 5 * T + 7, 3)]


def test_read_boundaries(ctx):
    """2 000 reads of 0 to 3 rows: many marks per word; empty reads first, last and several in a row"""
    rng = np.random.default_rng(41)
    lengths = [0, 0, 0] + rng.integers(0, 4, 2000).tolist() + [0, 0]
    offsets = offsets_of(lengths)
    pile = random_table(rng, int(offsets[-1]))
    segs, seg_off, reads = check_segments(ctx, pile, offsets, (1, 0, 1), device=True)
    assert reads["n_segs"].max() >= 1 and (reads["n_bases"] == np.array(lengths)).all()
    check_segments(ctx, pile, offsets, (12, 0, 2))
    # two adjacent all-good reads are two segments
    segs, _, reads = check_segments(ctx, table([7] * 130), offsets_of([64, 66]), (3, 3, 1), device=True)
    assert segs.tolist() == [(0, 0, 64, 0), (1, 0, 66, 0)] and reads["cls"].tolist() == [A.TRIM_WHOLE] * 2


def test_rules(ctx):
    # min_len at the run length - 1, the run length and the run length + 1
    depths = np.zeros(3 * T, np.int64)
    depths[T - 30:T + 40] = 4
    for min_len, kept in ((69, 1), (70, 1), (71, 0)):
        segs, _, reads = check_segments(ctx, table(depths), offsets_of([3 * T]), (3, 0, min_len))
        assert len(segs) == kept and reads["n_good"].tolist() == [70] and reads["cls"].tolist() == [A.TRIM_ENDS if kept else A.TRIM_NONE]
    # min_depth 1 and 2^32 - 1 on depths around both
    rng = np.random.default_rng(42)
    pile = np.zeros((2 * T + 5, 8), np.uint32)
    pile[:, A.PILE_A] = rng.choice(np.array([0, 1, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), pile.shape[0])
    pile[:, A.PILE_C] = rng.integers(0, 2, pile.shape[0])
    pile[:, A.PILE_ENDS] = rng.choice(np.array([0, 1, 0xFFFFFFFF], np.uint32), pile.shape[0])
    for rule in ((1, 0, 1), (0xFFFFFFFF, 0, 1), (0xFFFFFFFF, 1, 1), (1, 0xFFFFFFFF, 2), (2, 2, 1)):
        check_segments(ctx, pile, offsets_of([T, 0, T + 5]), rule, device=rule[1] == 1)
    # all bad and all good
    for depth, cls in ((2, A.TRIM_NONE), (3, A.TRIM_WHOLE)):
        segs, _, reads = check_segments(ctx, table([depth] * (2 * T + 1)), offsets_of([2 * T + 1]), (3, 3, 1), device=True)
        assert reads["cls"].tolist() == [cls] and len(segs) == (cls == A.TRIM_WHOLE)
    # LONGEST with ties: runs of equal length, the leftmost wins
    depths = np.zeros(T + 200, np.int64)
    for start in (5, 400, T - 25, T + 100):
        depths[start:start + 50] = 3
    want = reference_segments(table(depths), offsets_of([T + 200]), 3, 0, 1, True)
    assert want[0].tolist() == [(0, 5, 55, 0)] and want[2]["n_segs"].tolist() == [4]
    check_segments(ctx, table(depths), offsets_of([T + 200]), (3, 0, 1), device=True)


# ---- the interface ----------------------------------------------------------------------------------------------------------------
def _p(x):
    """the address of a numpy array, None as it is"""
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def test_count_only_and_capacity(ctx):
    rng = np.random.default_rng(43)
    offsets = offsets_of([70, 0, T + 3])
    pile = random_table(rng, int(offsets[-1]))
    want = reference_segments(pile, offsets, 12, 8, 2)
    n = len(want[0])
    assert n > 5
    p = A.PileSegParams(12, 8, 2, 0)

    def run(segs, cap):
        seg_off, reads, total = np.full(4, 99, np.uint64), np.zeros(3, TRIM), C.c_uint64(12345)
        rc = ctx.L.kmu_pile_segments(ctx.h, _p(pile), _p(offsets), 3, C.byref(p), A.MEM_HOST, _p(seg_off), _p(segs), cap, C.byref(total), _p(reads))
        assert seg_off.tolist() == want[1].tolist() and reads.tobytes() == want[2].tobytes() and total.value == n
        return rc
    assert run(None, 0) == 0                                                          # the count-only call
    segs = np.full(n + 2, 0xEE, np.uint8).repeat(16).view(SEG)
    assert run(segs, n) == 0 and segs[:n].tobytes() == want[0].tobytes() and (segs[n:].view(np.uint8) == 0xEE).all()   # cap exactly the total
    segs.view(np.uint8)[:] = 0xEE
    assert run(segs, n - 1) == A.E_BAD_ARG and (segs.view(np.uint8) == 0xEE).all()     # one short
    # either of the offsets and the summaries may be left out
    total = C.c_uint64(0)
    assert ctx.L.kmu_pile_segments(ctx.h, _p(pile), _p(offsets), 3, C.byref(p), A.MEM_HOST, None, _p(segs), n, C.byref(total), None) == 0
    assert segs[:n].tobytes() == want[0].tobytes()
    # no reads: one offset
    seg_off = np.full(2, 99, np.uint64)
    assert ctx.L.kmu_pile_segments(ctx.h, _p(pile), _p(offsets), 0, C.byref(p), A.MEM_HOST, _p(seg_off), None, 0, C.byref(total), None) == 0
    assert seg_off.tolist() == [0, 99] and total.value == 0


def test_every_bad_argument_of_the_segments(ctx):
    rng = np.random.default_rng(44)
    offsets = offsets_of([70, 200])
    pile = random_table(rng, 270)
    seg_off, segs, reads, total = np.full(3, 99, np.uint64), np.full(270 * 16, 0xEE, np.uint8), np.full(64, 0xEE, np.uint8), C.c_uint64(12345)
    base = dict(pile=pile, offsets=offsets, params=(3, 3, 1, 0), mem=A.MEM_HOST, seg_off=seg_off, segs=segs, total=total, reads=reads)

    def run(**kw):
        a = dict(base, **kw)
        p = A.PileSegParams(*a["params"]) if a["params"] is not None else None
        return ctx.L.kmu_pile_segments(ctx.h, _p(a["pile"]), _p(a["offsets"]), 2, C.byref(p) if p is not None else None, a["mem"], _p(a["seg_off"]),
                                       _p(a["segs"]), 270, C.byref(a["total"]) if a["total"] is not None else None, _p(a["reads"]))
    bad = [dict(pile=None), dict(offsets=None), dict(params=None), dict(total=None), dict(seg_off=None, segs=None, reads=None),
           dict(params=(0, 3, 1, 0)), dict(params=(3, 3, 0, 0)), dict(params=(3, 3, 1, 2)), dict(params=(3, 3, 1, 0x80000001)), dict(mem=7), dict(mem=-1)]
    for kw in bad:
        assert run(**kw) == A.E_BAD_ARG, sorted(kw)
        assert (seg_off == 99).all() and (segs == 0xEE).all() and (reads == 0xEE).all() and total.value == 12345, sorted(kw)
    want = reference_segments(pile, offsets, 3, 3, 1)
    assert run() == 0 and total.value == len(want[0]) and seg_off.tolist() == want[1].tolist() and reads.tobytes() == want[2].tobytes()
    assert segs[:16 * len(want[0])].tobytes() == want[0].tobytes()


# ---- kmu_extract_ranges -------------------------------------------------------------------------------------------------------------
def check_extract(ctx, bases, begin, end, device=True):
    import torch
    begin, end = np.asarray(begin, np.uint64), np.asarray(end, np.uint64)
    want = reference_extract(bases, begin, end)
    got = ctx.extract_ranges(bases, begin, end)
    assert got[0].dtype == np.uint8 and got[1].dtype == np.uint64
    assert got[1].tolist() == want[1].tolist() and got[0].tobytes() == want[0].tobytes()
    if device:
        d = ctx.extract_ranges(torch.from_numpy(bases).cuda(), torch.from_numpy(begin.view(np.int64)).cuda(), torch.from_numpy(end.view(np.int64)).cuda())
        assert d[0].is_cuda and d[1].is_cuda and d[1].dtype == torch.int64
        assert d[1].cpu().numpy().view(np.uint64).tolist() == want[1].tolist() and d[0].cpu().numpy().tobytes() == want[0].tobytes()
    return want


def test_extract_shapes(ctx):
    rng = np.random.default_rng(45)
    bases = rng.integers(0, 256, 4 * EXT_TILE + 77).astype(np.uint8)
    n = bases.size
    check_extract(ctx, bases, [5], [3 * EXT_TILE + 10])                                   # one range of several tiles
    start = rng.integers(0, n, 5000)
    check_extract(ctx, bases, start, start + 1)                                           # 5 000 one-byte ranges
    begin = rng.integers(0, n, 700)
    length = np.where(rng.integers(0, 3, 700) == 0, 0, rng.integers(0, 300, 700))
    length[100:250] = 0                                                                   # more than 64 empty ranges in a row
    end = np.minimum(begin + length, n)
    begin[5], end[5] = 0, n                                                               # the whole batch, among overlapping and unordered ranges
    begin[6], end[6] = begin[3], end[3]                                                   # a repeated range
    want = check_extract(ctx, bases, begin, end)
    assert int(want[1][-1]) > 3 * EXT_TILE
    check_extract(ctx, bases, [n, 0, n], [n, 0, n])                                       # begin = end = n_bases: nothing, three times
    check_extract(ctx, bases, [0], [EXT_TILE])                                            # exactly one tile
    check_extract(ctx, bases, [1, 0], [EXT_TILE, 1])                                      # a range that ends on a tile's last byte
    check_extract(ctx, bases[:0], [0, 0], [0, 0])                                         # an empty batch
    for k in (1, 63, 64, 65, EXT_TILE - 1, EXT_TILE, EXT_TILE + 1):                       # k + 1 offsets: one and two rounds of the 64-ary
        start = rng.integers(0, n, k)                                                     # search; at 4097 the second tile's first byte
        check_extract(ctx, bases, start, start + 1)                                       # lies in the last range
    length = np.array([EXT_TILE] + [0] * 130 + [10] + [0] * 70)                           # a tile that ends on a range's end, more than 64
    begin = rng.integers(0, n - EXT_TILE, length.size)                                    # empty ranges before the next byte, and empty
    want = check_extract(ctx, bases, begin, begin + length)                               # ranges behind the last byte
    assert int(want[1][-1]) == EXT_TILE + 10


def test_extract_every_alignment(ctx):
    """every source alignment 0 .. 7 against every destination alignment 0 .. 7, in one call: a filler range of d bytes puts the
    next range at destination alignment d (mod 8)"""
    rng = np.random.default_rng(46)
    bases = rng.integers(0, 256, 3000).astype(np.uint8)
    begin, end, at = [], [], 0
    for s in range(8):
        for d in range(8):
            fill = (d - at) % 8
            begin += [16, 8 * (10 + s + 8 * d) + s]
            end += [16 + fill, begin[-1] + 29 + s + d]
            at += fill + 29 + s + d
            assert (at - 29 - s - d) % 8 == d and begin[-1] % 8 == s
    check_extract(ctx, bases, begin, end)


def test_extract_refusals_leave_the_output_untouched(ctx):
    import torch
    bases = np.arange(100, dtype=np.uint8)
    for begin, end in (([0, 50, 10], [10, 49, 20]), ([0, 90], [10, 101]), ([101], [101]), ([2 ** 63], [2 ** 63 + 5])):
        b, e = np.array(begin, np.uint64), np.array(end, np.uint64)
        out, off, total = np.full(300, 0xEE, np.uint8), np.full(len(begin) + 1, 99, np.uint64), C.c_uint64(12345)
        assert ctx.L.kmu_extract_ranges(ctx.h, _p(bases), 100, _p(b), _p(e), len(begin), A.MEM_HOST, _p(off), _p(out), 300, C.byref(total)) == A.E_UNSUPPORTED
        assert (out == 0xEE).all() and (off == 99).all()
        d_out, d_off = torch.full((300,), 0x5A, dtype=torch.uint8, device="cuda"), torch.full((len(begin) + 1,), 99, dtype=torch.int64, device="cuda")
        d = [torch.from_numpy(x.view(t)).cuda() for x, t in ((bases, np.uint8), (b, np.int64), (e, np.int64))]
        rc = ctx.L.kmu_extract_ranges(ctx.h, C.c_void_p(d[0].data_ptr()), 100, C.c_void_p(d[1].data_ptr()), C.c_void_p(d[2].data_ptr()), len(begin),
                                      A.MEM_DEVICE, C.c_void_p(d_off.data_ptr()), C.c_void_p(d_out.data_ptr()), 300, C.byref(total))
        assert rc == A.E_UNSUPPORTED and (d_out == 0x5A).all().item() and (d_off == 99).all().item()
        with pytest.raises(lib.KmuError) as err:
            ctx.extract_ranges(bases, b, e)
        assert err.value.code == A.E_UNSUPPORTED
    # capacity: count-only, exact, one short; bad arguments
    b, e = np.array([10, 0], np.uint64), np.array([30, 5], np.uint64)
    out, off, total = np.full(40, 0xEE, np.uint8), np.full(3, 99, np.uint64), C.c_uint64(12345)
    assert ctx.L.kmu_extract_ranges(ctx.h, _p(bases), 100, _p(b), _p(e), 2, A.MEM_HOST, _p(off), None, 0, C.byref(total)) == 0
    assert total.value == 25 and off.tolist() == [0, 20, 25]
    off[:] = 99
    assert ctx.L.kmu_extract_ranges(ctx.h, _p(bases), 100, _p(b), _p(e), 2, A.MEM_HOST, _p(off), _p(out), 24, C.byref(total)) == A.E_BAD_ARG
    assert total.value == 25 and off.tolist() == [0, 20, 25] and (out == 0xEE).all()
    assert ctx.L.kmu_extract_ranges(ctx.h, _p(bases), 100, _p(b), _p(e), 2, A.MEM_HOST, _p(off), _p(out), 25, C.byref(total)) == 0
    assert out[:25].tolist() == list(range(10, 30)) + list(range(5)) and (out[25:] == 0xEE).all()
    out[:] = 0xEE
    total.value = 12345
    for kw in (dict(off=None), dict(total=None), dict(bases=None), dict(b=None), dict(e=None), dict(mem=7)):
        a = dict(dict(off=off, total=total, bases=bases, b=b, e=e, mem=A.MEM_HOST), **kw)
        off[:] = 99
        rc = ctx.L.kmu_extract_ranges(ctx.h, _p(a["bases"]), 100, _p(a["b"]), _p(a["e"]), 2, a["mem"], _p(a["off"]), _p(out), 40,
                                      C.byref(a["total"]) if a["total"] is not None else None)
        assert rc == A.E_BAD_ARG and (out == 0xEE).all() and (off == 99).all() and total.value == 12345, sorted(kw)
    check_extract(ctx, bases, b, e)   # the context goes on working


# ---- kmu_pile_consensus_pos -----------------------------------------------------------------------------------------------------------
def test_consensus_pos_of_every_row(ctx):
    import torch
    rng = np.random.default_rng(47)
    pile, call, ins_len, n_slots, ins, bases, offsets = rows = random_rows(rng, [0, 70, 0, 200, 130, 0], 16, with_slots=(0, 63, 64, 127, 128, 399))
    n = bases.size
    assert n_slots > 10 and n == 400
    every = np.arange(n + 1, dtype=np.uint64)
    want = reference_cons_pos(pile, call, ins_len, ins, bases, offsets, every)
    got = ctx.pile_consensus_pos(*rows, every)
    assert got.dtype == np.uint64 and got.tolist() == want.tolist()
    cons, coff = ctx.pile_consensus(*rows)
    assert int(got[-1]) == cons.size and ctx.pile_consensus_pos(*rows, offsets).tolist() == coff.tolist()   # rows = offsets: the read offsets
    assert coff.tolist() == reference_consensus(pile, call, ins_len, ins, bases, offsets)[1].tolist()
    perm = rng.permutation(n + 1).astype(np.uint64)[:150]                                                   # any order, repeats
    perm[:5] = n
    assert ctx.pile_consensus_pos(*rows, perm).tolist() == want[perm.astype(np.int64)].tolist()
    assert ctx.pile_consensus_pos(*rows, every[:0]).shape == (0,)
    dev = [torch.from_numpy(x.view(t)).cuda() for x, t in ((pile, np.int32), (call, np.uint8), (ins_len, np.uint8))]
    d = ctx.pile_consensus_pos(*dev, n_slots, torch.from_numpy(ins.view(np.int32)).cuda(), torch.from_numpy(bases).cuda(), offsets,
                               torch.from_numpy(every.view(np.int64)).cuda())
    assert d.is_cuda and d.dtype == torch.int64 and d.cpu().numpy().tolist() == want.tolist()
    # refusals: a row above n_bases, a wrong n_slots; the output stays as it was
    p, pos = A.ConsensusParams(0), np.full(3, 99, np.uint64)

    def raw(rows_q, n_slots_q, flags=0, mem=A.MEM_HOST, ins_q=ins):
        p.flags = flags
        return ctx.L.kmu_pile_consensus_pos(ctx.h, _p(pile), _p(call), _p(ins_len), n_slots_q, _p(ins_q), _p(bases), _p(offsets), len(offsets) - 1, C.byref(p),
                                            mem, _p(rows_q), 3, _p(pos))
    assert raw(np.array([0, n + 1, 5], np.uint64), n_slots) == A.E_UNSUPPORTED and (pos == 99).all()
    assert raw(np.array([0, 1, 2], np.uint64), n_slots + 1, ins_q=np.zeros((n_slots + 1, 4), np.uint32)) == A.E_UNSUPPORTED and (pos == 99).all()
    assert raw(np.array([0, 1, 2], np.uint64), n_slots, flags=1) == A.E_BAD_ARG and raw(np.array([0, 1, 2], np.uint64), n_slots, mem=7) == A.E_BAD_ARG
    assert raw(None, n_slots) == A.E_BAD_ARG and raw(np.array([0, 1, 2], np.uint64), n_slots, ins_q=None) == A.E_BAD_ARG and (pos == 99).all()
    assert raw(np.array([0, n, 5], np.uint64), n_slots) == 0 and pos.tolist() == want[[0, n, 5]].tolist()
    with pytest.raises(lib.KmuError) as err:
        ctx.pile_consensus_pos(*rows, np.array([n + 1], np.uint64))
    assert err.value.code == A.E_UNSUPPORTED


# ---- planted truth --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(ctx):
    """templates A and B of 600 bases; ten copies of each as mutate(X[:400]) + mutate(X[400:]) at 5 % errors, so the row of template
    position 400 is known in every copy; one chimera mutate(A[:400]) + mutate(B[400:]) with its join at row na; one copy of A with 100
    random bases appended.  Hand-made chains: whole against whole inside a family; the chimera's two parts against the matching
    parts of every copy of their parents; the tailed read's clean part against whole copies of A."""
    rng = np.random.default_rng(71)
    tmpl = [rng.choice(ACGT, 600).astype(np.uint8) for _ in range(2)]

    def two_parts(left, right):
        a, b = mutate(rng, left[:400], 0.05)[0], mutate(rng, right[400:], 0.05)[0]
        return bytes(a).decode() + bytes(b).decode(), len(a)
    reads, cut = [], []
    for x in tmpl:
        for _ in range(10):
            s, c = two_parts(x, x)
            reads.append(s)
            cut.append(c)
    chimera, na = two_parts(tmpl[0], tmpl[1])
    clean = two_parts(tmpl[0], tmpl[0])[0]
    reads += [chimera, clean + bytes(rng.choice(ACGT, 100).astype(np.uint8)).decode()]
    CH, TL = 20, 21
    recs = [(r, q, 0, 0, len(reads[r]), 0, len(reads[q])) for f in (0, 10) for r in range(f, f + 10) for q in range(r + 1, f + 10)]
    recs += [(CH, i, 0, 0, na, 0, cut[i]) for i in range(10)]
    recs += [(CH, i, 0, na, len(chimera), cut[i], len(reads[i])) for i in range(10, 20)]
    recs += [(TL, i, 0, 0, len(clean), 0, len(reads[i])) for i in range(10)]
    bases, offsets = batch(reads)
    chains = chain_recs(recs)
    band = 64
    while True:   # (an alignment that is not exact at this band: a wider band, never a weaker assertion)
        aln, ops, op_off = ctx.chain_cigar(chains, bases, offsets, band=band)
        if ((aln["flags"] & (A.ALN_PATH | A.ALN_EXACT)) == (A.ALN_PATH | A.ALN_EXACT)).all() or band >= 1024:
            break
        band *= 2
    assert ((aln["flags"] & (A.ALN_PATH | A.ALN_EXACT)) == (A.ALN_PATH | A.ALN_EXACT)).all()
    pile = ctx.chain_pileup(chains, aln, ops, op_off, bases, offsets)[0]
    return dict(reads=reads, na=na, clean=len(clean), bases=bases, offsets=offsets, chains=chains, aln=aln, ops=ops, op_off=op_off, pile=pile, CH=CH, TL=TL)


def test_planted_chimera_tail_and_plain_copies(ctx, planted):
    pile, offsets, na, CH, TL = (planted[k] for k in ("pile", "offsets", "na", "CH", "TL"))
    n_ch, n_tl = len(planted["reads"][CH]), len(planted["reads"][TL])
    segs, seg_off, reads = check_segments(ctx, pile, offsets, (3, 3, 100), device=True)
    mine = segs[segs["read"] == CH]
    assert reads["cls"][CH] == A.TRIM_SPLIT and [(int(s["start"]), int(s["end"])) for s in mine] == [(0, na), (na, n_ch)]
    tail = segs[segs["read"] == TL]
    assert reads["cls"][TL] == A.TRIM_ENDS and [(int(s["start"]), int(s["end"])) for s in tail] == [(0, n_tl - 100)] and planted["clean"] == n_tl - 100
    assert (reads["cls"][:20] == A.TRIM_WHOLE).all() and reads["inner_bad"].tolist() == [0] * 22
    # depth alone does not see the join
    _, _, depth_only = check_segments(ctx, pile, offsets, (3, 0, 100))
    assert depth_only["cls"][CH] == A.TRIM_WHOLE and depth_only["cls"][TL] == A.TRIM_ENDS
    # min_depth 1: the tail would be kept if it had any depth, which it has not
    _, _, one = check_segments(ctx, pile, offsets, (1, 1, 100))
    assert one["cls"][TL] == A.TRIM_ENDS and (int(one["best_start"][TL]), int(one["best_end"][TL])) == (0, n_tl - 100)


def test_planted_trim_and_correct_trim_routes(ctx, planted):
    import torch
    p = planted
    pile, bases, offsets, na, CH = p["pile"], p["bases"], p["offsets"], p["na"], p["CH"]
    # trim_reads: the step-by-step route and the references, on the device's own table
    out, out_off, segs, reads = minimizer.trim_reads(ctx, pile, bases, offsets, min_depth=3, min_len=100)
    want_segs, _, want_reads = reference_segments(pile, offsets, 3, 3, 100)
    same(segs, want_segs, "segs")
    same(reads, want_reads, "reads")
    beg = offsets[want_segs["read"]]
    want = reference_extract(bases, beg + want_segs["start"], beg + want_segs["end"])
    assert out.tobytes() == want[0].tobytes() and out_off.tolist() == want[1].tolist() and out_off.shape[0] == 22 + 1 + 1   # the chimera is two reads
    d = minimizer.trim_reads(ctx, torch.from_numpy(pile.view(np.int32)).cuda(), torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.view(np.int64)).cuda(),
                             min_depth=3, min_len=100)
    assert all(x.is_cuda for x in d) and [x.cpu().numpy().tobytes() for x in d] == [out.tobytes(), out_off.tobytes(), segs.tobytes(), reads.tobytes()]
    best = minimizer.trim_reads(ctx, pile, bases, offsets, min_depth=3, min_len=100, longest=True)
    assert best[1].shape[0] == 22 + 1 and len(best[2]) == 22
    # the corrected pieces: calls, slots and consensus of the same table, the positions of the segments' rows, the ranges of the consensus
    call, _ = ctx.pile_call(pile, bases, offsets, min_depth=3)
    ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=16)
    ins = ctx.chain_pile_ins(p["chains"], p["aln"], p["ops"], p["op_off"], bases, offsets, ins_len, n_slots)[0]
    cons, coff = ctx.pile_consensus(pile, call, ins_len, n_slots, ins, bases, offsets)
    rows = np.concatenate([beg + want_segs["start"], beg + want_segs["end"]])
    pos = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, bases, offsets, rows)
    assert pos.tolist() == reference_cons_pos(pile, call, ins_len, ins, bases, offsets, rows).tolist()
    n = len(want_segs)
    pieces, piece_off = ctx.extract_ranges(cons, pos[:n], pos[n:])
    want_pieces = reference_extract(cons, pos[:n], pos[n:])
    assert pieces.tobytes() == want_pieces[0].tobytes() and piece_off.tolist() == want_pieces[1].tolist()
    at = int(offsets[CH])
    q = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, bases, offsets, np.array([at, at + na, int(offsets[CH + 1])], np.uint64)).astype(np.int64)
    k = int(np.nonzero(want_segs["read"] == CH)[0][0])
    assert np.diff(piece_off.astype(np.int64))[k:k + 2].tolist() == [int(q[1] - q[0]), int(q[2] - q[1])]
    assert int(q[0]) == int(coff[CH]) and int(q[2]) == int(coff[CH + 1])


def test_correct_trim_reads_equals_the_step_by_step_route(ctx, planted):
    """correct_trim_reads finds the chains itself; its batch equals the step-by-step route on the same chains, the references on the
    device's own tables, and on resident arrays everything stays on the device and holds the same bytes"""
    import torch
    bases, offsets = planted["bases"], planted["offsets"]
    kw = dict(min_depth=3, max_ins=8, min_len=50)
    out, out_off, segs, reads, trims = minimizer.correct_trim_reads(ctx, bases, offsets, 15, 10, **kw)
    chains, aln, ops, op_off = minimizer.read_cigars(ctx, bases, offsets, 15, 10)
    pile, _ = minimizer.pileup_chains(ctx, chains, aln, ops, op_off, bases, offsets)
    call, want_reads = ctx.pile_call(pile, bases, offsets, min_depth=3)
    ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=8)
    ins, _ = minimizer.insertions_chains(ctx, chains, aln, ops, op_off, bases, offsets, ins_len, n_slots)
    cons, _ = reference_consensus(pile, call, ins_len, ins, bases, offsets)
    want_segs, _, want_trims = reference_segments(pile, offsets, 3, 3, 50)
    same(segs, want_segs, "segs")
    same(trims, want_trims, "trims")
    assert reads.tobytes() == want_reads.tobytes() and len(segs) > 0
    beg = offsets[want_segs["read"]]
    pos = reference_cons_pos(pile, call, ins_len, ins, bases, offsets, np.concatenate([beg + want_segs["start"], beg + want_segs["end"]]))
    want = reference_extract(cons, pos[:len(segs)], pos[len(segs):])
    assert out.tobytes() == want[0].tobytes() and out_off.tolist() == want[1].tolist()
    d = minimizer.correct_trim_reads(ctx, torch.from_numpy(bases).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda(), 15, 10, **kw)
    assert all(x.is_cuda for x in d)
    assert [x.cpu().numpy().tobytes() for x in d] == [out.tobytes(), out_off.tobytes(), segs.tobytes(), reads.tobytes(), trims.tobytes()]


def test_the_kernels_that_ran(ctx):
    rng = np.random.default_rng(48)
    offsets = offsets_of([70, 0, T + 3])
    pile = random_table(rng, int(offsets[-1]))
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        segs, _, _ = ctx.pile_segments(pile, offsets, 10, 0, 1, longest=True)
        beg = offsets[segs["read"]]
        ctx.extract_ranges(np.zeros(int(offsets[-1]), np.uint8), beg + segs["start"], beg + segs["end"])
        ctx.pile_consensus_pos(*random_rows(rng, [70, 30], 16), np.array([0, 100], np.uint64))
        ran = set(ctx.profile_get())
        assert {"k_seg_marks", "k_seg_count", "k_seg_write", "k_seg_keep", "k_seg_place", "k_seg_reads", "k_seg_longest", "k_ext_lens", "k_ext_offsets",
                "k_ext_copy", "k_cons_count", "k_cons_pos_check", "k_cons_pos"} <= ran and "k_cons_write" not in ran
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

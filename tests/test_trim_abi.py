"""-m "not gpu": the host side of read trimming -- `reference_segments`, `reference_extract` and `reference_cons_pos`: the contracts of
kmu_pile_segments, kmu_extract_ranges and kmu_pile_consensus_pos (include/kmu.h) as plain numpy, which tests/test_gpu_pile_segments.py
compares the device against; hand cases worked out on paper, written as functions of the implementation; the symbols and their
bindings, the constants and struct sizes, refusals that need no device, and the minimizer wrappers on a stub context."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import batch  # noqa: E402
from test_consensus_abi import depth_of, reference_consensus, slot_base  # noqa: E402
from test_pileup_abi import reference_call  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_TILE = 1024   # rows per tile of the segment pass (kmu_seg_core.h); tests/test_gpu_pile_segments.py builds its edges from it
EXT_TILE = 4096   # output bytes per tile of kmu_extract_ranges


# ---- the references ---------------------------------------------------------------------------------------------------------------
def reference_segments(pile, offsets, min_depth, min_span, min_len, longest=False):
    """(segs, seg_offsets, reads) of kmu_pile_segments by the text of include/kmu.h: A.PILE_SEG_DTYPE records, uint64 [n_reads + 1],
    A.READ_TRIM_DTYPE records"""
    pile = np.asarray(pile).reshape(-1, A.PILE_COLS)
    depth = depth_of(pile)
    ends = pile.astype(np.int64)[:, A.PILE_ENDS] & 0xFFFFFFFF
    good, span = depth >= min_depth, np.maximum(depth - ends, 0)
    off = np.asarray(offsets).astype(np.int64)
    segs, seg_off, reads = [], [0], []
    for r in range(len(off) - 1):
        beg, end = int(off[r]), int(off[r + 1])
        runs, g = [], beg
        while g < end:
            if not good[g]:
                g += 1
                continue
            s = g
            g += 1
            while g < end and good[g] and max(int(span[g]), int(span[g - 1])) >= min_span:
                g += 1
            runs.append((s - beg, g - beg))
        kept = [x for x in runs if x[1] - x[0] >= min_len]
        best = (0, 0)
        for x in kept:
            if x[1] - x[0] > best[1] - best[0]:
                best = x
        total = sum(e - s for s, e in kept)
        cls = A.TRIM_NONE if not kept else A.TRIM_SPLIT if len(kept) > 1 else A.TRIM_WHOLE if total == end - beg else A.TRIM_ENDS
        reads.append((end - beg, int(good[beg:end].sum()), len(kept), total, best[0], best[1], (kept[-1][1] - kept[0][0] - total) if kept else 0, cls))
        listed = [(r, s, e, k) for k, (s, e) in enumerate(kept)]
        if longest:
            listed = [x for x in listed if (x[1], x[2]) == best][:1]
        segs += listed
        seg_off.append(len(segs))
    return (np.array(segs, np.dtype(A.PILE_SEG_DTYPE)) if segs else np.zeros(0, np.dtype(A.PILE_SEG_DTYPE)), np.array(seg_off, np.uint64),
            np.array(reads, np.dtype(A.READ_TRIM_DTYPE)) if reads else np.zeros(0, np.dtype(A.READ_TRIM_DTYPE)))


class Unsupported(Exception):
    pass


def reference_extract(bases, begin, end):
    """(out, out_offsets) of kmu_extract_ranges; Unsupported for a range with begin > end or end > n_bases"""
    bases = np.asarray(bases)
    b, e = np.asarray(begin).astype(np.uint64), np.asarray(end).astype(np.uint64)
    if (b > e).any() or (e > bases.size).any():
        raise Unsupported()
    parts = [bases[int(x):int(y)] for x, y in zip(b, e)]
    off = np.zeros(len(parts) + 1, np.uint64)
    off[1:] = np.cumsum([p.size for p in parts])
    return (np.concatenate(parts) if parts else bases[:0]).astype(np.uint8), off


def reference_cons_pos(pile, call, ins_len, ins, bases, offsets, rows):
    """pos of kmu_pile_consensus_pos: the consensus bytes of the rows before every named row; Unsupported for a row above n_bases"""
    depth, s = depth_of(pile), slot_base(ins_len)
    ins = np.asarray(ins).astype(np.int64) & 0xFFFFFFFF
    n = len(bases)
    rows = np.asarray(rows).astype(np.uint64)
    if (rows > n).any():
        raise Unsupported()
    row_end = np.zeros(n + 1, np.int64)
    for g in range(n):
        length = 0 if (int(call[g]) & 7) == A.PILE_DEL else 1
        for k in range(int(ins_len[g])):
            if not 2 * int(ins[s[g] + k].sum()) > int(depth[g]):
                break
            length += 1
        row_end[g + 1] = row_end[g] + length
    return row_end[rows.astype(np.int64)].astype(np.uint64)


# ---- hand cases -------------------------------------------------------------------------------------------------------------------
def table(depths, ends=None):
    """a table whose rows have these depths (all in column A) and these ENDS"""
    pile = np.zeros((len(depths), A.PILE_COLS), np.uint32)
    pile[:, A.PILE_A] = depths
    if ends is not None:
        pile[:, A.PILE_ENDS] = ends
    return pile


def as_lists(result):
    segs, seg_off, reads = result
    return [tuple(int(x) for x in s) for s in np.asarray(segs).tolist()], np.asarray(seg_off).tolist(), [tuple(int(x) for x in r) for r in np.asarray(reads).tolist()]


def segment_cases(segments):
    """the hand cases of kmu_pile_segments; segments(pile, offsets, min_depth, min_span, min_len, longest) -> (segs, seg_offsets, reads):
    reference_segments here, the device in tests/test_gpu_pile_segments.py"""
    def by_hand(depths, ends, lengths, *rule, longest=False):
        off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        return as_lists(segments(table(depths, ends), off, *rule, longest))
    W, E, S, N = A.TRIM_WHOLE, A.TRIM_ENDS, A.TRIM_SPLIT, A.TRIM_NONE
    # one read, depth 3 everywhere, nothing ends inside: whole                 n_bases good segs kept best inner cls
    assert by_hand([3] * 6, [3, 0, 0, 0, 0, 3], [6], 3, 0, 1) == ([(0, 0, 6, 0)], [0, 1], [(6, 6, 1, 6, 0, 6, 0, W)])
    # ... the first and last row have depth - ends = 0, their neighbours 3: linked from either side at min_span 3
    assert by_hand([3] * 6, [3, 0, 0, 0, 0, 3], [6], 3, 3, 1) == ([(0, 0, 6, 0)], [0, 1], [(6, 6, 1, 6, 0, 6, 0, W)])
    # a flush join between rows 2 and 3: three partners end at 2, three begin at 3
    join = ([3] * 6, [3, 0, 3, 3, 0, 3], [6])
    assert by_hand(*join, 3, 0, 1) == ([(0, 0, 6, 0)], [0, 1], [(6, 6, 1, 6, 0, 6, 0, W)])
    assert by_hand(*join, 3, 1, 1) == ([(0, 0, 3, 0), (0, 3, 6, 1)], [0, 2], [(6, 6, 2, 6, 0, 3, 0, S)])   # equal lengths: the leftmost is best
    assert by_hand(*join, 3, 1, 1, longest=True) == ([(0, 0, 3, 0)], [0, 1], [(6, 6, 2, 6, 0, 3, 0, S)])
    assert by_hand(*join, 3, 1, 4) == ([], [0, 0], [(6, 6, 0, 0, 0, 0, 0, N)])                             # min_len above both
    # ends larger than depth: the difference is clamped at 0, not wrapped
    assert by_hand([3, 3], [9, 9], [2], 3, 1, 1) == ([(0, 0, 1, 0), (0, 1, 2, 1)], [0, 2], [(2, 2, 2, 2, 0, 1, 0, S)])
    # uncovered ends and a hole: [1, 4) and [6, 8) of 9 rows; min_len 3 keeps only the first
    holes = ([0, 3, 3, 3, 1, 0, 4, 4, 2], None, [9])
    assert by_hand(*holes, 3, 0, 1) == ([(0, 1, 4, 0), (0, 6, 8, 1)], [0, 2], [(9, 5, 2, 5, 1, 4, 2, S)])
    assert by_hand(*holes, 3, 0, 3) == ([(0, 1, 4, 0)], [0, 1], [(9, 5, 1, 3, 1, 4, 0, E)])
    assert by_hand(*holes, 3, 0, 2, longest=True) == ([(0, 1, 4, 0)], [0, 1], [(9, 5, 2, 5, 1, 4, 2, S)])
    assert by_hand(*holes, 1, 0, 1) == ([(0, 1, 5, 0), (0, 6, 9, 1)], [0, 2], [(9, 7, 2, 7, 1, 5, 1, S)])
    # the longest is the second: its rank stays 1 in the LONGEST list
    assert by_hand([3, 3, 0, 3, 3, 3], None, [6], 3, 0, 1, longest=True) == ([(0, 3, 6, 1)], [0, 1], [(6, 5, 2, 5, 3, 6, 1, S)])
    # two adjacent all-good reads are two segments; empty reads first, between and last
    assert by_hand([5] * 5, None, [0, 2, 0, 0, 3, 0], 3, 0, 1) == (
        [(1, 0, 2, 0), (4, 0, 3, 0)], [0, 0, 1, 1, 1, 2, 2],
        [(0, 0, 0, 0, 0, 0, 0, N), (2, 2, 1, 2, 0, 2, 0, W), (0, 0, 0, 0, 0, 0, 0, N), (0, 0, 0, 0, 0, 0, 0, N), (3, 3, 1, 3, 0, 3, 0, W), (0, 0, 0, 0, 0, 0, 0, N)])
    # all bad
    assert by_hand([2] * 4, None, [1, 3], 3, 0, 1) == ([], [0, 0, 0], [(1, 0, 0, 0, 0, 0, 0, N), (3, 0, 0, 0, 0, 0, 0, N)])


def deep_row_case(segments):
    """A = 2^32 - 1, C = 1: depth 2^32, good at min_depth 2^32 - 1, and not 0"""
    pile = np.zeros((3, A.PILE_COLS), np.uint32)
    pile[:, A.PILE_A] = [0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF]
    pile[0, A.PILE_C] = 1
    off = np.array([0, 3], np.uint64)
    assert as_lists(segments(pile, off, 0xFFFFFFFF, 0, 1, False)) == ([(0, 0, 1, 0), (0, 2, 3, 1)], [0, 2], [(3, 2, 2, 2, 0, 1, 1, A.TRIM_SPLIT)])
    assert as_lists(segments(pile, off, 1, 0, 1, False))[0] == [(0, 0, 3, 0)]
    # ends 2^32 - 1 below depth 2^32: span 1
    pile[:, A.PILE_ENDS] = 0xFFFFFFFF
    assert as_lists(segments(pile, off, 1, 1, 1, False))[0] == [(0, 0, 2, 0), (0, 2, 3, 1)]   # rows 1 and 2 have span 0


def extract_cases(extract):
    """extract(bases, begin, end) -> (out, out_offsets)"""
    bases = np.frombuffer(b"ACGTacgtNN", np.uint8)

    def by_hand(ranges):
        out, off = extract(bases, np.array([r[0] for r in ranges], np.uint64), np.array([r[1] for r in ranges], np.uint64))
        return np.asarray(out).tobytes(), np.asarray(off).tolist()
    assert by_hand([(0, 4), (4, 8)]) == (b"ACGTacgt", [0, 4, 8])
    assert by_hand([(8, 10), (2, 2), (0, 3), (1, 3), (8, 10), (10, 10)]) == (b"NNACGCGNN", [0, 2, 2, 5, 7, 9, 9])   # unordered, empty, overlapping, repeated
    assert by_hand([(10, 10)]) == (b"", [0, 0])
    assert by_hand([]) == (b"", [0])
    assert by_hand([(0, 10)]) == (b"ACGTacgtNN", [0, 10])


def test_segment_rules_by_hand():
    segment_cases(reference_segments)
    deep_row_case(reference_segments)


def test_extract_by_hand():
    extract_cases(reference_extract)
    for bad in ([(3, 2)], [(0, 11)], [(0, 4), (11, 11)]):
        with pytest.raises(Unsupported):
            reference_extract(np.zeros(10, np.uint8), [b for b, _ in bad], [e for _, e in bad])


def test_reference_cons_pos_of_the_offsets_is_the_consensus_offsets():
    rng = np.random.default_rng(5)
    bases, offsets = batch(["".join(rng.choice(list("ACGTn"), n)) for n in (0, 70, 1, 0, 130)])
    n = bases.size
    pile = rng.integers(0, 4, (n, 8)).astype(np.uint32)
    call = reference_call(pile, bases, offsets, 2)[0]
    ins_len = rng.integers(0, 3, n).astype(np.uint8)
    ins = rng.integers(0, 4, (int(ins_len.sum()), 4)).astype(np.uint32)
    cons, coff = reference_consensus(pile, call, ins_len, ins, bases, offsets)
    assert reference_cons_pos(pile, call, ins_len, ins, bases, offsets, offsets).tolist() == coff.tolist()
    every = reference_cons_pos(pile, call, ins_len, ins, bases, offsets, np.arange(n + 1))
    assert every[0] == 0 and every[-1] == cons.size and (np.diff(every.astype(np.int64)) >= 0).all() and ((call & 7) == A.PILE_DEL).any()
    with pytest.raises(Unsupported):
        reference_cons_pos(pile, call, ins_len, ins, bases, offsets, [n + 1])


# ---- the symbols and their surroundings -------------------------------------------------------------------------------------------
def test_symbols_and_bindings():
    """fails without the feature: the symbols are missing"""
    L = lib.load()
    for name in ("kmu_pile_segments", "kmu_extract_ranges", "kmu_pile_consensus_pos"):
        assert name in lib.SYMBOLS and hasattr(L, name)
    assert len(L.kmu_pile_segments.argtypes) == 11 and len(L.kmu_extract_ranges.argtypes) == 11 and len(L.kmu_pile_consensus_pos.argtypes) == 14
    assert callable(lib.Context.pile_segments) and callable(lib.Context.extract_ranges) and callable(lib.Context.pile_consensus_pos)
    assert callable(minimizer.trim_reads) and callable(minimizer.correct_trim_reads)


def test_constants_and_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()

    def define(name):
        return int(re.search(r"#define %s\s+(\d+)u?\s" % name, txt).group(1))
    assert define("KMU_SEG_LONGEST") == A.SEG_LONGEST == 1
    assert [define("KMU_TRIM_" + n) for n in ("WHOLE", "ENDS", "SPLIT", "NONE")] == [A.TRIM_WHOLE, A.TRIM_ENDS, A.TRIM_SPLIT, A.TRIM_NONE] == [0, 1, 2, 3]
    assert C.sizeof(A.PileSegParams) == 16 and C.sizeof(A.PileSeg) == 16 and C.sizeof(A.ReadTrim) == 32
    assert np.dtype(A.PILE_SEG_DTYPE).itemsize == 16 and np.dtype(A.READ_TRIM_DTYPE).itemsize == 32
    for struct, dtype, name in ((A.PileSegParams, None, r"typedef struct kmu_pile_seg_params \{(.*?)\}"), (A.PileSeg, A.PILE_SEG_DTYPE, r"typedef struct \{([^}]*?)\} kmu_pile_seg;"),
                                (A.ReadTrim, A.READ_TRIM_DTYPE, r"typedef struct \{([^}]*?)\} kmu_read_trim;")):
        fields = re.findall(r"uint32_t (\w+);", re.search(name, txt, re.S).group(1))
        assert [n for n, _ in struct._fields_] == fields
        assert dtype is None or [n for n, _ in dtype] == fields
    tail = txt[txt.index("int kmu_pile_consensus("):]
    assert tail.index("int kmu_pile_segments(") < tail.index("int kmu_extract_ranges(") < tail.index("int kmu_pile_consensus_pos(")
    core = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_seg_core.h")).read()
    assert int(re.search(r"constexpr uint32_t SEG_TRIPS = (\d+);", core).group(1)) * 64 == SEG_TILE
    gather = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_gather_core.h")).read()
    assert int(re.search(r"constexpr uint32_t GATHER_TILE = (\d+);", gather).group(1)) == EXT_TILE
    # the step from a tile's offset to a row exists once
    cons = open(os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_pile_consensus.hip")).read()
    assert cons.count("uint64_t cons_pos_at(") == 1 and cons.count("= cons_pos_at(") == 2


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(64, np.uint8)
    a = arr.ctypes.data
    n = C.c_uint64(99)
    seg, cons = A.PileSegParams(3, 3, 1, 0), A.ConsensusParams(0)
    assert L.kmu_pile_segments(None, a, a, 1, C.byref(seg), A.MEM_HOST, a, a, 4, C.byref(n), a) == A.E_BAD_ARG
    assert L.kmu_pile_segments(None, None, None, 0, None, 7, None, None, 0, None, None) == A.E_BAD_ARG
    assert L.kmu_extract_ranges(None, a, 8, a, a, 1, A.MEM_HOST, a, a, 64, C.byref(n)) == A.E_BAD_ARG
    assert L.kmu_extract_ranges(None, None, 0, None, None, 0, 7, None, None, 0, None) == A.E_BAD_ARG
    assert L.kmu_pile_consensus_pos(None, a, a, a, 0, a, a, a, 1, C.byref(cons), A.MEM_HOST, a, 1, a) == A.E_BAD_ARG
    assert L.kmu_pile_consensus_pos(None, None, None, None, 0, None, None, None, 0, None, 7, None, 0, None) == A.E_BAD_ARG
    assert not arr.any() and n.value == 99


# ---- the wrappers on a stub context -----------------------------------------------------------------------------------------------
class _StubContext:
    def __init__(self):
        self.seen = []

    def chain_pileup(self, *args, **kw):
        return "pile", "pile"

    def pile_call(self, pile, bases, offsets, min_depth=3):
        return "call", "reads"

    def pile_ins_plan(self, pile, call, max_ins=16):
        return "len", 11

    def chain_pile_ins(self, *args, **kw):
        return "ins", "ins"

    def pile_consensus(self, *args):
        return "cons", "coff"

    def pile_segments(self, pile, offsets, min_depth=3, min_span=None, min_len=1, longest=False):
        self.seen.append(("segments", pile, min_depth, min_span, min_len, longest))
        segs = np.array([(0, 1, 3, 0), (1, 0, 2, 0)], np.dtype(A.PILE_SEG_DTYPE))
        return segs, "seg_off", "trims"

    def pile_consensus_pos(self, pile, call, ins_len, n_slots, ins, bases, offsets, rows):
        self.seen.append(("pos", pile, call, ins_len, n_slots, ins, bases, np.asarray(rows).tolist()))
        return np.asarray(rows) * 2

    def extract_ranges(self, bases, begin, end):
        self.seen.append(("extract", bases, np.asarray(begin).tolist(), np.asarray(end).tolist()))
        return "out", "out_off"


def test_wrappers_pass_everything_on(monkeypatch):
    stub = _StubContext()
    offsets = np.array([0, 10, 20], np.uint64)
    out = minimizer.trim_reads(stub, "pile", "b", offsets, min_depth=4, min_len=2, longest=True)
    assert out[:2] == ("out", "out_off") and out[3] == "trims" and out[2]["end"].tolist() == [3, 2]
    assert stub.seen == [("segments", "pile", 4, None, 2, True), ("extract", "b", [1, 10], [3, 12])]   # offsets[read] + start / end
    monkeypatch.setattr(minimizer, "read_cigars", lambda *a: ("ch", "aln", "ops", "off"))
    stub.seen.clear()
    out = minimizer.correct_trim_reads(stub, "b", offsets, 15, 10, min_depth=2, max_ins=7, min_span=1, min_len=5)
    assert out[:2] == ("out", "out_off") and out[3:] == ("reads", "trims")
    assert stub.seen == [("segments", "pile", 2, 1, 5, False), ("pos", "pile", "call", "len", 11, "ins", "b", [1, 10, 3, 12]),
                         ("extract", "cons", [2, 20], [6, 24])]

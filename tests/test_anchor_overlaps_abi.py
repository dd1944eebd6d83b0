"""-m "not gpu": the host side of kmu_anchor_overlaps -- the symbol and its binding, the constants and the record, the record
layout of anchor.read_overlaps on a stub context, and `reference_overlaps`: the rules of include/kmu.h as plain Python over
dicts keyed by (read_a, read_b, strand, diag), which tests/test_gpu_anchor_overlaps.py compares the device against.  The reference
is itself tested here on three cases whose answers are written out by hand."""
import ctypes as C
import os
import re

import numpy as np

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype(A.OVERLAP_DTYPE)


def reference_overlaps(pairs, dist, off_q, off_db=None, strands=2, band=1, min_score=1, upper=False):
    """the records of kmu_anchor_overlaps (a structured array of A.OVERLAP_DTYPE), by the text of include/kmu.h"""
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    off_q = np.asarray(off_q).astype(np.int64)
    off_db = off_q if off_db is None else np.asarray(off_db).astype(np.int64)
    weight = np.ones(pairs.shape[0], np.int64) if dist is None else np.asarray(dist).reshape(-1, 3)[:, 0].astype(np.int64)
    read_a = np.searchsorted(off_q, pairs[:, 0], side="right") - 1
    read_b = np.searchsorted(off_db, pairs[:, 1], side="right") - 1
    slice_a, slice_b = pairs[:, 0] - off_q[read_a], pairs[:, 1] - off_db[read_b]
    diags = {}  # (read_a, read_b, strand, diag) -> [W, V, slice_a_min, slice_a_max]
    by_pair = {}  # (read_a, read_b) -> {(strand, diag)}
    for ra, rb, sa, sb, w in zip(read_a.tolist(), read_b.tolist(), slice_a.tolist(), slice_b.tolist(), weight.tolist()):
        for s in range(strands):
            d = sa - sb if s == 0 else sa + sb
            e = diags.setdefault((ra, rb, s, d), [0, 0, sa, sa])
            e[0] += w
            e[1] += 1
            e[2], e[3] = min(e[2], sa), max(e[3], sa)
            by_pair.setdefault((ra, rb), set()).add((s, d))
    out = []
    for (ra, rb) in sorted(by_pair):
        if upper and not ra < rb:
            continue
        best = None
        for (s, d) in sorted(by_pair[(ra, rb)]):  # strand 0 first, then ascending d: the first of the largest is the winner
            band_runs = [diags[(ra, rb, s, e)] for e in range(d, d + band + 1) if (ra, rb, s, e) in diags]
            score = sum(r[0] for r in band_runs)
            if best is None or score > best[0]:
                best = (score, s, d, sum(r[1] for r in band_runs), min(r[2] for r in band_runs), max(r[3] for r in band_runs))
        if best[0] >= min_score:
            out.append((ra, rb, best[1], best[2], min(best[0], 0xFFFFFFFF), best[3], best[4], best[5]))
    return np.array(out, REC).reshape(-1)


def test_symbol_is_exported_and_bound():
    L = lib.load()
    assert "kmu_anchor_overlaps" in lib.SYMBOLS and hasattr(L, "kmu_anchor_overlaps")
    assert len(L.kmu_anchor_overlaps.argtypes) == 16
    assert callable(getattr(lib.Context, "anchor_overlaps")) and callable(anchor.read_overlaps)


def test_constants_and_record_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    assert int(re.search(r"#define KMU_OVL_MAX_BAND (\d+)", txt).group(1)) == A.OVL_MAX_BAND == 8
    assert int(re.search(r"#define KMU_OVL_UPPER (\d+)u", txt).group(1)) == A.OVL_UPPER == 1
    assert "int kmu_anchor_overlaps(kmu_ctx *ctx" in txt
    body = re.search(r"typedef struct \{([^}]*)\} kmu_overlap;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"(u?int32_t)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in A.OVERLAP_DTYPE] == [n for n, _ in A.Overlap._fields_]
    assert [t for t, _ in fields] == ["int32_t" if n == "diag" else "uint32_t" for n, _ in A.OVERLAP_DTYPE]
    assert C.sizeof(A.Overlap) == 32 and REC.itemsize == 32
    assert [REC.fields[n][1] for n, _ in A.OVERLAP_DTYPE] == [getattr(A.Overlap, n).offset for n, _ in A.OVERLAP_DTYPE]


# ---- the reference on cases worked out by hand: reads of 10 rows each, row = 10 * read + slice -----------------------------------
OFF = np.arange(0, 50, 10, dtype=np.uint64)  # 4 reads


def test_reference_a_tie_between_strands_goes_to_strand_0():
    # read 0 x read 1: (slice 2, slice 1) and (slice 3, slice 0).  strand 0: d = 1 and d = 3; strand 1: d = 3 twice.
    pairs = np.array([[2, 11], [3, 10]], np.uint32)
    # band 2: S_0(1) = W_0(1) + W_0(3) = 2 = S_1(3): strand 0 wins, from d = 1, with both pairs in the band
    got = reference_overlaps(pairs, None, OFF, strands=2, band=2)
    assert got.tolist() == [(0, 1, 0, 1, 2, 2, 2, 3)]
    # band 1: S_0(1) = S_0(3) = 1 < S_1(3) = 2
    got = reference_overlaps(pairs, None, OFF, strands=2, band=1)
    assert got.tolist() == [(0, 1, 1, 3, 2, 2, 2, 3)]
    # one strand, band 0: the two diagonals tie at 1, the smaller d wins
    got = reference_overlaps(pairs, None, OFF, strands=1, band=0)
    assert got.tolist() == [(0, 1, 0, 1, 1, 1, 2, 2)]


def test_reference_a_band_stops_at_the_read_pair():
    # read 0 x read 1 on d = 5 (weight 1); read 0 x read 2 on d = 6 (weight 10) and d = 8 (weight 3)
    pairs = np.array([[5, 10], [7, 21], [8, 20]], np.uint32)
    dist = np.array([[1, 9, 9], [10, 9, 9], [3, 9, 9]], np.uint32)
    got = reference_overlaps(pairs, dist, OFF, strands=1, band=1)
    assert got.tolist() == [(0, 1, 0, 5, 1, 1, 5, 5), (0, 2, 0, 6, 10, 1, 7, 7)]
    got = reference_overlaps(pairs, dist, OFF, strands=1, band=2)  # 6 .. 8 holds both runs of (0, 2); (0, 1) still has 1
    assert got.tolist() == [(0, 1, 0, 5, 1, 1, 5, 5), (0, 2, 0, 6, 13, 2, 7, 8)]
    got = reference_overlaps(pairs, dist, OFF, strands=1, band=2, min_score=2)
    assert got.tolist() == [(0, 2, 0, 6, 13, 2, 7, 8)]


def test_reference_a_negative_diagonal_and_upper():
    # read 1 slice 0 x read 3 slice 7, and slice 1 x slice 9: d = -7 and -8; the mirrored pairs (3, 1) have d = +7, +8
    pairs = np.array([[10, 37], [11, 39], [37, 10], [39, 11], [12, 12]], np.uint32)
    got = reference_overlaps(pairs, None, OFF, strands=1, band=1)
    assert got.tolist() == [(1, 1, 0, 0, 1, 1, 2, 2), (1, 3, 0, -8, 2, 2, 0, 1), (3, 1, 0, 7, 2, 2, 7, 9)]
    got = reference_overlaps(pairs, None, OFF, strands=1, band=1, upper=True)
    assert got.tolist() == [(1, 3, 0, -8, 2, 2, 0, 1)]
    assert got["diag"].dtype == np.int32
    assert reference_overlaps(np.zeros((0, 2), np.uint32), None, OFF).shape == (0,)


# ---- read_overlaps on a stub context --------------------------------------------------------------------------------------------
class _StubContext:
    """anchor_match and anchor_overlaps return canned arrays and remember what they were asked"""

    def anchor_match(self, hashes_q, hashes_db, n_keys=1, min_common=1, group_q=None, group_db=None):
        self.match = (hashes_q, hashes_db, n_keys, min_common, group_q, group_db)
        self.pairs = np.array([[0, 3], [2, 4], [3, 0], [4, 2]], np.uint32)
        self.dist = np.array([[5, 8, 7], [1, 8, 8], [4, 8, 6], [1, 8, 8]], np.uint32)
        return self.pairs, self.dist

    def anchor_overlaps(self, pairs, dist, row_offsets_q, row_offsets_db=None, strands=2, band=1, min_score=1, upper=False):
        self.ovl = (pairs, dist, row_offsets_q, row_offsets_db, strands, band, min_score, upper)
        return np.array([(0, 1, 0, -2, 9, 3, 1, 2), (0, 2, 1, 5, 4, 1, 0, 0)], REC)


def test_read_overlaps_record_layout():
    params = anchor.AnchorsGeneratorParameters("x", 400, 8, 21, 100)  # stride 300
    hashes = np.zeros((7, 8), np.uint64)
    row_offsets = np.array([0, 3, 5, 7], np.uint64)
    stub = _StubContext()
    rec = anchor.read_overlaps(stub, hashes, row_offsets, params, n_keys=4, min_common=2, strands=2, band=3, min_score=5, first_readnum=20)
    assert rec.dtype == np.int64 and rec.shape == (2, 8)
    # readnum_a, readnum_b, strand, offset in bases, score, votes, first and last slicepos_a
    assert rec.tolist() == [[20, 21, 0, -600, 9, 3, 300, 600], [20, 22, 1, 1500, 4, 1, 0, 0]]
    q, db, n_keys, min_common, gq, gdb = stub.match
    assert q is hashes and db is hashes and (n_keys, min_common) == (4, 2)
    assert gq.dtype == np.uint32 and gq.tolist() == [0, 0, 0, 1, 1, 2, 2] and gdb.tolist() == gq.tolist()
    pairs, dist, off_q, off_db, strands, band, min_score, upper = stub.ovl
    assert pairs is stub.pairs and dist is stub.dist and off_db is None
    assert off_q.dtype == np.uint64 and off_q.tolist() == [0, 3, 5, 7]
    assert (strands, band, min_score, upper) == (2, 3, 5, True)
    # the defaults: one key, band 1, both strands, a score of at least 2
    anchor.read_overlaps(stub, hashes, row_offsets, params)
    assert stub.match[2:4] == (1, 1) and stub.ovl[4:] == (2, 1, 2, True)

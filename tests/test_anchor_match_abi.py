"""-m "not gpu": the host side of the anchor matching -- the symbol and its binding, the constant, rows_to_slices, and the
record layout of match_read_anchors on a stub context that returns canned pairs."""
import os
import re

import numpy as np

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_exported_and_bound():
    L = lib.load()
    assert "kmu_anchor_match" in lib.SYMBOLS and hasattr(L, "kmu_anchor_match")
    assert len(L.kmu_anchor_match.argtypes) == 15
    assert callable(getattr(lib.Context, "anchor_match"))


def test_constant_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    tile = int(re.search(r"#define KMU_ANCHOR_SORT_TILE (\d+)", txt).group(1))
    assert tile == A.ANCHOR_SORT_TILE and tile % 64 == 0
    assert "int kmu_anchor_match(kmu_ctx *ctx" in txt


def test_rows_to_slices():
    row_offsets = np.array([0, 3, 3, 4, 9], np.uint64)  # read 1 has no row
    rows = np.array([0, 2, 3, 4, 8, 1], np.uint32)
    readnum, slicepos = anchor.rows_to_slices(rows, row_offsets, 250)
    assert readnum.tolist() == [0, 0, 2, 3, 3, 0] and slicepos.tolist() == [0, 500, 0, 0, 1000, 250]
    readnum, slicepos = anchor.rows_to_slices(rows, row_offsets, 30, first_readnum=7)
    assert readnum.tolist() == [7, 7, 9, 10, 10, 7] and slicepos.tolist() == [0, 60, 0, 0, 120, 30]
    readnum, slicepos = anchor.rows_to_slices(np.zeros(0, np.uint32), row_offsets, 30)
    assert readnum.shape == (0,) and slicepos.shape == (0,)


class _StubContext:
    """anchor_match returns canned pairs and remembers what it was asked"""

    def anchor_match(self, hashes_q, hashes_db, n_keys=1, min_common=1, group_q=None, group_db=None):
        self.asked = (hashes_q, hashes_db, n_keys, min_common, group_q, group_db)
        pairs = np.array([[0, 3], [2, 4], [3, 0], [4, 2]], np.uint32)
        dist = np.array([[5, 8, 7], [1, 8, 8], [4, 8, 6], [1, 8, 8]], np.uint32)
        return pairs, dist


def test_match_read_anchors_record_layout():
    params = anchor.AnchorsGeneratorParameters("x", 400, 8, 21, 100)  # stride 300
    hashes = np.zeros((5, 8), np.uint64)
    row_offsets = np.array([0, 3, 5], np.uint64)
    stub = _StubContext()
    rec = anchor.match_read_anchors(stub, hashes, row_offsets, params, n_keys=4, min_common=2, first_readnum=20)
    assert rec.dtype == np.int64 and rec.shape == (4, 6)
    # readnum_a, slicepos_a, readnum_b, slicepos_b, common, total
    assert rec.tolist() == [[20, 0, 21, 0, 5, 8], [20, 600, 21, 300, 1, 8], [21, 0, 20, 0, 4, 8], [21, 300, 20, 600, 1, 8]]
    q, db, n_keys, min_common, gq, gdb = stub.asked
    assert q is hashes and db is hashes and (n_keys, min_common) == (4, 2)
    assert gq.dtype == np.uint32 and gq.tolist() == [0, 0, 0, 1, 1] and gdb.tolist() == gq.tolist()

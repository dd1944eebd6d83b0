"""-m "not gpu": the host side of the anchor index -- the symbols and their bindings, the info record against the header,
max_occ_for_fraction on histograms written out by hand, and the route that match_read_anchors / read_overlaps take on a stub
context: anchor_match without a mask, anchor_index(...).match(..., max_occ) with one."""
import ctypes as C
import os
import re

import numpy as np

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype(A.OVERLAP_DTYPE)


def test_symbols_are_exported_and_bound():
    L = lib.load()
    want = {"kmu_anchor_index_create": 8, "kmu_anchor_index_destroy": 1, "kmu_anchor_index_info": 2,
            "kmu_anchor_index_occupancy": 4, "kmu_anchor_index_match": 11}
    for name, n_args in want.items():
        assert name in lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args, name
    assert L.kmu_anchor_index_destroy.restype is None
    assert callable(getattr(lib.Context, "anchor_index"))
    for method in ("match", "occupancy", "info", "close", "__enter__", "__exit__"):
        assert callable(getattr(lib.AnchorIndex, method))
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    for name in want:
        assert re.search(r"\b%s\(" % name, txt), name
    assert "typedef struct kmu_anchor_index kmu_anchor_index;" in txt


def test_info_record_matches_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} kmu_anchor_index_info_t;", txt).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"(uint32_t|uint64_t)\s+([^;]+);", body) for n in names.split(",")]
    assert [n for _, n in fields] == [n for n, _ in A.AnchorIndexInfo._fields_]
    assert [t for t, _ in fields] == ["uint64_t" if c is C.c_uint64 else "uint32_t" for _, c in A.AnchorIndexInfo._fields_]
    # natural alignment: four u32, two u64, two u32, one u64
    assert C.sizeof(A.AnchorIndexInfo) == 48
    offsets = {n: getattr(A.AnchorIndexInfo, n).offset for n, _ in A.AnchorIndexInfo._fields_}
    assert offsets == {"ndb": 0, "m": 4, "n_keys": 8, "has_groups": 12, "n_entries": 16, "n_distinct": 24, "max_occupancy": 32,
                       "pad": 36, "device_bytes": 40}


def test_max_occ_for_fraction():
    f = anchor.max_occ_for_fraction
    hist = np.array([0, 5, 3, 0, 2], np.uint64)  # ten keys: five in one row, three in two, two in four
    assert f(hist, 0) == 4        # nothing may lie above: the largest occupancy present
    assert f(hist, 0.19) == 4     # two keys above 3 are 20 %
    assert f(hist, 0.2) == 2      # a tie: "at most" -- and the smallest such c, 2 rather than 3
    assert f(hist, 0.49) == 2
    assert f(hist, 0.5) == 1      # five keys above 1 are exactly half
    assert f(hist, 0.99) == 1
    assert f(hist, 1) == 0 and f(hist, 2.5) == 0
    assert isinstance(f(hist, 0.2), int)
    assert f(np.zeros(6, np.uint64), 0.3) == 0 and f(np.zeros(6, np.uint64), 0) == 0  # an index without a key
    assert f(np.array([0, 7], np.uint64), 0) == 1 and f(np.array([0, 7], np.uint64), 0.5) == 1  # all keys alike
    assert f([0, 1000, 0, 1], 9e-4) == 3 and f([0, 1000, 0, 1], 1e-3) == 1  # a list will do; 1 key of 1001 lies above 1
    assert f(np.array([0, 9, 1], np.int64), 0.1) == 1


class _StubIndex:
    def __init__(self, owner, args):
        self.owner, self.args, self.closed = owner, args, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        self.closed = True

    def match(self, hashes_q, group_q=None, min_common=1, max_occ=0):
        self.asked = (hashes_q, group_q, min_common, max_occ)
        return self.owner.pairs, self.owner.dist


class _StubContext:
    """anchor_match (which takes no max_occ), anchor_index and anchor_overlaps return canned arrays and remember what they were asked"""
    pairs = np.array([[0, 3], [2, 4], [3, 0], [4, 2]], np.uint32)
    dist = np.array([[5, 8, 7], [1, 8, 8], [4, 8, 6], [1, 8, 8]], np.uint32)

    def __init__(self):
        self.matched, self.indexes = [], []

    def anchor_match(self, hashes_q, hashes_db, n_keys=1, min_common=1, group_q=None, group_db=None):
        self.matched.append((hashes_q, hashes_db, n_keys, min_common, group_q, group_db))
        return self.pairs, self.dist

    def anchor_index(self, hashes_db, n_keys=1, group_db=None):
        self.indexes.append(_StubIndex(self, (hashes_db, n_keys, group_db)))
        return self.indexes[-1]

    def anchor_overlaps(self, pairs, dist, row_offsets_q, row_offsets_db=None, strands=2, band=1, min_score=1, upper=False):
        self.ovl = (pairs, dist)
        return np.array([(0, 1, 0, -2, 9, 3, 1, 2)], REC)


PARAMS = anchor.AnchorsGeneratorParameters("x", 400, 8, 21, 100)  # stride 300
HASHES = np.zeros((5, 8), np.uint64)
ROW_OFFSETS = np.array([0, 3, 5], np.uint64)
RECORDS = [[20, 0, 21, 0, 5, 8], [20, 600, 21, 300, 1, 8], [21, 0, 20, 0, 4, 8], [21, 300, 20, 600, 1, 8]]


def test_without_a_mask_the_join_is_anchor_match():
    for kw in ({}, {"max_occ": 0}):
        stub = _StubContext()
        rec = anchor.match_read_anchors(stub, HASHES, ROW_OFFSETS, PARAMS, n_keys=4, min_common=2, first_readnum=20, **kw)
        assert rec.tolist() == RECORDS
        assert len(stub.matched) == 1 and not stub.indexes
        assert stub.matched[0][0] is HASHES and stub.matched[0][1] is HASHES and stub.matched[0][2:4] == (4, 2)
        ro = anchor.read_overlaps(stub, HASHES, ROW_OFFSETS, PARAMS, n_keys=2, **kw)
        assert ro.tolist() == [[0, 1, 0, -600, 9, 3, 300, 600]]
        assert len(stub.matched) == 2 and not stub.indexes and stub.matched[1][2:4] == (2, 1)


def test_with_a_mask_the_join_goes_through_an_index():
    stub = _StubContext()
    rec = anchor.match_read_anchors(stub, HASHES, ROW_OFFSETS, PARAMS, n_keys=4, min_common=2, first_readnum=20, max_occ=5)
    assert rec.tolist() == RECORDS
    assert not stub.matched and len(stub.indexes) == 1
    index = stub.indexes[0]
    hashes_db, n_keys, group_db = index.args
    assert hashes_db is HASHES and n_keys == 4
    assert group_db.dtype == np.uint32 and group_db.tolist() == [0, 0, 0, 1, 1]
    hashes_q, group_q, min_common, max_occ = index.asked
    assert hashes_q is HASHES and group_q is group_db and (min_common, max_occ) == (2, 5)
    assert index.closed  # the index of one call does not outlive it
    ro = anchor.read_overlaps(stub, HASHES, ROW_OFFSETS, PARAMS, n_keys=2, max_occ=5)
    assert ro.tolist() == [[0, 1, 0, -600, 9, 3, 300, 600]]
    assert not stub.matched and len(stub.indexes) == 2
    index = stub.indexes[1]
    assert index.args[1] == 2 and index.asked[2:] == (1, 5) and index.closed
    assert stub.ovl[0] is stub.pairs and stub.ovl[1] is stub.dist

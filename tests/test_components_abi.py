"""-m "not gpu": the host side of kmu_components / kmu_components_knn -- the symbols and their binding, the prototypes in the
header, what anchor.read_clusters passes on (on a stub context), and the references that tests/test_gpu_components.py compares the
device against: `reference_components` (a plain union-find by the text of include/kmu.h) and the two functions that pick the edges
that count.  The references are themselves tested here on cases whose answers are written out by hand."""
import os
import re

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib, sketching

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype(A.OVERLAP_DTYPE)


def reference_components(n_nodes, u, v):
    """(label, cluster, size, members) of the undirected graph over 0 .. n_nodes - 1 with the edges (u[e], v[e]); self loops and
    edges with an end >= n_nodes are skipped.  uint32 arrays; size has n_components entries."""
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(u).astype(np.int64).tolist(), np.asarray(v).astype(np.int64).tolist()):
        if a == b or not 0 <= a < n_nodes or not 0 <= b < n_nodes:
            continue
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)  # the smaller root stays: the root of a component is its smallest node
    label = np.array([find(x) for x in range(n_nodes)], np.uint32).reshape(-1)
    roots = np.flatnonzero(label == np.arange(n_nodes))  # ascending: the order of the smallest member
    rank = np.zeros(n_nodes + 1, np.int64)
    rank[roots] = np.arange(roots.size)
    cluster = rank[label.astype(np.int64)].astype(np.uint32)
    size = np.bincount(cluster, minlength=roots.size).astype(np.uint32)
    members = np.lexsort((np.arange(n_nodes), cluster)).astype(np.uint32)
    return label, cluster, size, members


def reference_edges_of(records, stride, weight_at, min_weight):
    """(u, v) of the records that count: rows of `stride` uint32 words, word weight_at >= min_weight unless weight_at is 0"""
    words = np.ascontiguousarray(records).reshape(-1).view(np.uint32).reshape(-1, stride).astype(np.int64)
    keep = np.ones(words.shape[0], bool) if weight_at == 0 else words[:, weight_at] >= min_weight
    return words[keep, 0], words[keep, 1]


def reference_edges_of_knn(idx, eq, min_eq):
    """(u, v) of the list entries that count: (i, idx[i, j]) with eq[i, j] >= min_eq (eq None: all of them)"""
    idx = np.asarray(idx).view(np.uint32).astype(np.int64)
    u = np.repeat(np.arange(idx.shape[0]), idx.shape[1]).reshape(idx.shape)
    keep = np.ones(idx.shape, bool) if eq is None else np.asarray(eq).view(np.uint16).astype(np.int64) >= min_eq
    return u[keep], idx[keep]


# ---- the symbols ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_bound():
    L = lib.load()
    for name, n_args in (("kmu_components", 13), ("kmu_components_knn", 12)):
        assert name in lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args
    assert callable(lib.Context.components) and callable(lib.Context.components_knn)
    assert callable(anchor.read_clusters) and callable(sketching.neighbour_clusters)
    assert lib.Components._fields == ("label", "cluster", "size", "members", "n_components")


def test_the_header_carries_both_prototypes():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int kmu_components(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *edges, uint64_t n_edges, uint32_t stride, "
            "uint32_t weight_at, uint32_t min_weight, int mem, uint32_t *label_out, uint32_t *cluster_out, uint32_t *size_out, "
            "uint32_t *members_out, uint32_t *n_components_out);") in flat
    assert ("int kmu_components_knn(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *idx, const uint16_t *eq, uint32_t k, "
            "uint32_t min_eq, int mem, uint32_t *label_out, uint32_t *cluster_out, uint32_t *size_out, uint32_t *members_out, "
            "uint32_t *n_components_out);") in flat
    doc = re.sub(r"\s*\n \*\s*", " ", txt)  # the comment as running text
    for rule in ("the smallest node of v's component", "never used as an index", "A pure function of the inputs",
                 "Duplicate edges and edges given in both directions change nothing"):
        assert rule in doc


# ---- the reference on cases worked out by hand ---------------------------------------------------------------------------------------
def test_reference_a_path_given_in_reverse_order():
    # 0 - 1 - 2 - 3 - 4, last edge first
    label, cluster, size, members = reference_components(5, [3, 2, 1, 0], [4, 3, 2, 1])
    assert label.tolist() == [0] * 5 and cluster.tolist() == [0] * 5 and size.tolist() == [5] and members.tolist() == [0, 1, 2, 3, 4]
    assert all(x.dtype == np.uint32 for x in (label, cluster, size, members))


def test_reference_two_components_and_an_isolated_node():
    # {1, 4, 5} and {0, 3, 6}; 2 alone.  A self loop on 2, the edge 4 - 5 twice (once reversed), an edge to node 7 of 7 nodes
    u = [5, 2, 6, 4, 5, 3, 2, 0xFFFFFFFF]
    v = [1, 2, 3, 5, 4, 0, 7, 1]
    label, cluster, size, members = reference_components(7, u, v)
    assert label.tolist() == [0, 1, 2, 0, 1, 1, 0]
    assert cluster.tolist() == [0, 1, 2, 0, 1, 1, 0]
    assert size.tolist() == [3, 3, 1]
    assert members.tolist() == [0, 3, 6, 1, 4, 5, 2]


def test_reference_an_empty_edge_list():
    label, cluster, size, members = reference_components(4, [], [])
    assert label.tolist() == [0, 1, 2, 3] and cluster.tolist() == [0, 1, 2, 3] and size.tolist() == [1] * 4 and members.tolist() == [0, 1, 2, 3]
    label, cluster, size, members = reference_components(0, [], [])
    assert label.shape == cluster.shape == size.shape == members.shape == (0,)


def test_reference_edges_of_records():
    # stride 3, the weight in word 2: 6, 7, 8 around min_weight 7
    rec = np.array([[0, 1, 6], [1, 2, 7], [2, 3, 8]], np.uint32)
    assert [x.tolist() for x in reference_edges_of(rec, 3, 2, 7)] == [[1, 2], [2, 3]]
    assert [x.tolist() for x in reference_edges_of(rec, 3, 2, 6)] == [[0, 1, 2], [1, 2, 3]]
    assert [x.tolist() for x in reference_edges_of(rec, 3, 2, 9)] == [[], []]
    assert [x.tolist() for x in reference_edges_of(rec, 3, 0, 9)] == [[0, 1, 2], [1, 2, 3]]  # weight_at 0: min_weight is not looked at
    # overlap records as they are: score is word 4, votes word 5; a weight above 2^31 is unsigned
    ovl = np.array([(0, 1, 0, -3, 5, 2, 0, 1), (1, 2, 1, 4, 0x90000000, 9, 0, 0)], REC)
    assert [x.tolist() for x in reference_edges_of(ovl, 8, 4, 6)] == [[1], [2]]
    assert [x.tolist() for x in reference_edges_of(ovl, 8, 5, 2)] == [[0, 1], [1, 2]]
    assert [x.tolist() for x in reference_edges_of(ovl, 8, 5, 3)] == [[1], [2]]
    # pairs: stride 2
    assert [x.tolist() for x in reference_edges_of(np.array([[4, 2], [2, 0]], np.uint32), 2, 0, 0)] == [[4, 2], [2, 0]]


def test_reference_edges_of_neighbour_lists():
    idx = np.array([[1, 2], [0, A.KNN_NONE], [0, 1]], np.uint32)
    eq = np.array([[9, 4], [9, 0], [4, 5]], np.uint16)
    assert [x.tolist() for x in reference_edges_of_knn(idx, eq, 5)] == [[0, 1, 2], [1, 0, 1]]
    assert [x.tolist() for x in reference_edges_of_knn(idx, eq, 4)] == [[0, 0, 1, 2, 2], [1, 2, 0, 0, 1]]
    assert [x.tolist() for x in reference_edges_of_knn(idx, eq, 6)] == [[0, 1], [1, 0]]
    u, v = reference_edges_of_knn(idx, None, 0)  # the entry that does not exist is an edge to node 2^32 - 1, dropped by the range rule
    assert v.tolist() == [1, 2, 0, A.KNN_NONE, 0, 1]
    assert reference_components(3, u, v)[0].tolist() == [0, 0, 0]
    u, v = reference_edges_of_knn(idx, eq, 6)
    assert reference_components(3, u, v)[0].tolist() == [0, 0, 2]
    # the same bits as signed tensors hand them over
    assert [x.tolist() for x in reference_edges_of_knn(idx.view(np.int32), eq.view(np.int16), 5)] == [[0, 1, 2], [1, 0, 1]]


def test_min_eq_for_identity():
    assert sketching.min_eq_for_identity(0.9, 10) == 9  # 0.9 * 10 is 9.000000000000002 in binary
    assert sketching.min_eq_for_identity(0.9, 200) == 180 and sketching.min_eq_for_identity(0.901, 200) == 181
    assert sketching.min_eq_for_identity(0.0, 64) == 0 and sketching.min_eq_for_identity(1.0, 64) == 64
    assert sketching.min_eq_for_identity(1 / 3, 3) == 1 and sketching.min_eq_for_identity(0.34, 3) == 2


# ---- read_clusters on a stub context ----------------------------------------------------------------------------------------------
class _StubContext:
    """anchor_match, anchor_overlaps and components return canned arrays and remember what they were asked"""

    def anchor_match(self, hashes_q, hashes_db, n_keys=1, min_common=1, group_q=None, group_db=None):
        self.match = (hashes_q, hashes_db, n_keys, min_common, group_q, group_db)
        self.pairs = np.array([[0, 3], [3, 0]], np.uint32)
        self.dist = np.array([[5, 8, 7], [4, 8, 6]], np.uint32)
        return self.pairs, self.dist

    def anchor_overlaps(self, pairs, dist, row_offsets_q, row_offsets_db=None, strands=2, band=1, min_score=1, upper=False):
        self.ovl = (pairs, dist, row_offsets_q, row_offsets_db, strands, band, min_score, upper)
        self.rec = np.array([(0, 1, 0, -2, 9, 3, 1, 2)], REC)
        return self.rec

    def components(self, edges, n_nodes, weight_at=0, min_weight=0, want=("cluster", "size", "members"), count=True):
        self.cc = (edges, n_nodes, weight_at, min_weight, tuple(want), count)
        u32 = lambda x: np.array(x, np.uint32)  # noqa: E731
        return lib.Components(u32([0, 0, 2]), u32([0, 0, 1]), u32([2, 1]), u32([0, 1, 2]) if "members" in want else None, 2)


def test_read_clusters_passes_the_records_on_as_they_are():
    params = anchor.AnchorsGeneratorParameters("x", 400, 8, 21, 100)
    hashes = np.zeros((7, 8), np.uint64)
    row_offsets = np.array([0, 3, 5, 7], np.uint64)
    stub = _StubContext()
    cluster, sizes = anchor.read_clusters(stub, hashes, row_offsets, params, n_keys=4, min_common=2, strands=1, band=3, min_score=5)
    assert cluster.dtype == np.int64 and cluster.tolist() == [0, 0, 1] and sizes.dtype == np.int64 and sizes.tolist() == [2, 1]
    q, db, n_keys, min_common, gq, gdb = stub.match
    assert q is hashes and db is hashes and (n_keys, min_common) == (4, 2) and gq.tolist() == [0, 0, 0, 1, 1, 2, 2] == gdb.tolist()
    pairs, dist, off_q, off_db, strands, band, min_score, upper = stub.ovl
    assert pairs is stub.pairs and dist is stub.dist and off_q.tolist() == [0, 3, 5, 7] and off_db is None
    assert (strands, band, min_score, upper) == (1, 3, 5, True)
    edges, n_nodes, weight_at, min_weight, want, count = stub.cc
    assert edges is stub.rec and edges.dtype.itemsize == 4 * 8  # the records themselves: stride 8
    assert (n_nodes, weight_at, min_weight, count) == (3, 4, 5, True) and want == ("cluster", "size")
    # by votes: word 5 decides, and the vote drops nothing on its own
    out = anchor.read_clusters(stub, hashes, row_offsets, params, min_score=3, by="votes", want_members=True, first_readnum=10)
    assert len(out) == 3 and out[2].dtype == np.int64 and out[2].tolist() == [10, 11, 12]
    assert stub.ovl[4:] == (2, 1, 0, True) and stub.cc[1:5] == (3, 5, 3, ("cluster", "size", "members"))
    # the defaults are read_overlaps': one key, band 1, both strands, a score of at least 2
    anchor.read_clusters(stub, hashes, row_offsets, params)
    assert stub.match[2:4] == (1, 1) and stub.ovl[4:] == (2, 1, 2, True) and stub.cc[2:4] == (4, 2)
    with pytest.raises(ValueError):
        anchor.read_clusters(stub, hashes, row_offsets, params, by="diag")

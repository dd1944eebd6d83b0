"""-m gpu: kmu_components / kmu_components_knn against reference_components (tests/test_components_abi.py: a plain union-find by the
text of include/kmu.h), whole arrays compared exactly.  Unless a case says otherwise it first asserts that the reference has at
least two components and one of more than one node: a case without either would show nothing.

Sizes: a wave has 64 lanes and a workgroup 256; the member lists are sorted in tiles of T = ANCHOR_SORT_TILE nodes and by the bytes
that n_nodes - 1 can reach (a second radix pass from 257 nodes on, a third from 65537 on); the device scan over the root flags
changes kernels above 32768 nodes."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib
from kmerutils_amd import sketching as S
from test_components_abi import REC, reference_components, reference_edges_of, reference_edges_of_knn

pytestmark = pytest.mark.gpu
T = A.ANCHOR_SORT_TILE
NONE = A.KNN_NONE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def assert_shows_something(want, single=False):
    size = want[2]
    if single:
        assert size.tolist() == [want[0].size]
    else:
        assert size.size >= 2 and size.max() > 1, "the case has %d components, the largest of %d" % (size.size, size.max() if size.size else 0)


def assert_same(got, want):
    label, cluster, size, members = want
    assert got.n_components == size.size
    for name, g, w in (("label", got.label, label), ("cluster", got.cluster, cluster), ("size", got.size, size), ("members", got.members, members)):
        g = np.asarray(g.cpu().numpy() if hasattr(g, "cpu") else g).view(np.uint32)
        assert g.shape == w.shape, name
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s differs at %s: got %s, want %s" % (name, bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def check(ctx, n_nodes, edges, weight_at=0, min_weight=0, single=False):
    """ctx.components on records (a [n, stride] array or overlap records) against the reference over the edges that count"""
    stride = 8 if edges.dtype.names else edges.shape[1]
    want = reference_components(n_nodes, *reference_edges_of(edges, stride, weight_at, min_weight))
    assert_shows_something(want, single)
    got = ctx.components(edges, n_nodes, weight_at=weight_at, min_weight=min_weight)
    assert all(isinstance(x, np.ndarray) and x.dtype == np.uint32 for x in got[:4])
    assert_same(got, want)
    return got


def pairs_of(u, v):
    return np.ascontiguousarray(np.stack([np.asarray(u), np.asarray(v)], axis=1).astype(np.uint32))


def random_pairs(rng, n_nodes, n_edges, among=None):
    return pairs_of(rng.integers(0, among or n_nodes, n_edges), rng.integers(0, among or n_nodes, n_edges))


# ---- node counts around the wave, the workgroup, the sort tile and the scan's change of kernel ----------------------------------------
@pytest.mark.parametrize("n_nodes", [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 32767, 32768, 32769, 65536, 65537])
def test_node_counts(ctx, n_nodes):
    rng = np.random.default_rng(n_nodes)
    # about n_nodes random edges: a few large components, many small ones, isolated nodes
    check(ctx, n_nodes, random_pairs(rng, n_nodes, n_nodes), single=n_nodes == 1)


# ---- deep trees: a single path, where path halving and hooks race and a stale read of parent would show -------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_one_path(ctx, order):
    n = 5000
    at = {"ascending": np.arange(n - 1), "descending": np.arange(n - 1)[::-1],
          "shuffled": np.random.default_rng(5).permutation(n - 1)}[order]
    got = check(ctx, n, pairs_of(at, at + 1), single=True)
    assert got.label.max() == 0 and got.size.tolist() == [n]
    check(ctx, n, pairs_of(at + 1, at), single=True)  # every edge the other way round


# ---- contention ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hub", ["first", "last"])
def test_star(ctx, hub):
    leaves = 20_000
    n = leaves + 1
    if hub == "first":
        edges = pairs_of(np.zeros(leaves, np.int64), np.arange(1, n))
    else:  # every hook lowers the root of the hub's tree again
        edges = pairs_of(np.arange(leaves), np.full(leaves, leaves))
    check(ctx, n, edges[np.random.default_rng(6).permutation(leaves)], single=True)


def test_disjoint_triangles(ctx):
    n_tri = 4000
    rng = np.random.default_rng(7)
    nodes = rng.permutation(3 * n_tri).reshape(n_tri, 3)  # the corners of a triangle are anywhere
    edges = pairs_of(np.concatenate([nodes[:, 0], nodes[:, 1], nodes[:, 2]]), np.concatenate([nodes[:, 1], nodes[:, 2], nodes[:, 0]]))
    got = check(ctx, 3 * n_tri, edges[rng.permutation(3 * n_tri)])
    assert got.n_components == n_tri and (got.size == 3).all()


# ---- one giant component with leftovers; shared by the cases that need a real graph -------------------------------------------------
@pytest.fixture(scope="module")
def giant():
    rng = np.random.default_rng(8)
    n_nodes = 50_000
    edges = random_pairs(rng, n_nodes, 200_000, among=40_000)
    want = reference_components(n_nodes, edges[:, 0], edges[:, 1])
    assert_shows_something(want)
    assert want[2].max() > 39_000 and want[2].size > 10_000  # the giant component; the 10 000 isolated nodes
    return n_nodes, edges, want


def test_giant_component_with_leftovers(ctx, giant):
    n_nodes, edges, want = giant
    assert_same(ctx.components(edges, n_nodes), want)


def test_the_result_is_bit_identical_from_run_to_run_and_under_a_permutation(ctx, giant):
    n_nodes, edges, want = giant
    first = ctx.components(edges, n_nodes)
    assert_same(first, want)
    again = ctx.components(edges, n_nodes)
    perm = np.random.default_rng(9).permutation(edges.shape[0])
    moved = ctx.components(np.ascontiguousarray(edges[perm]), n_nodes)
    for other in (again, moved):
        assert other.n_components == first.n_components
        for a, b in zip(first[:4], other[:4]):
            assert a.tobytes() == b.tobytes()


def test_optional_outputs(ctx, giant):
    n_nodes, edges, want = giant
    every = ("cluster", "size", "members")
    for left_out in every:
        got = ctx.components(edges, n_nodes, want=tuple(w for w in every if w != left_out))
        assert getattr(got, left_out) is None and got.n_components == want[2].size
        for name, w in zip(("label",) + every, want):
            if name != left_out:
                assert np.array_equal(getattr(got, name), w), name
    # without the count: nothing crosses to the host, and size comes back whole
    got = ctx.components(edges, n_nodes, count=False)
    assert got.n_components is None and got.size.shape == (n_nodes,)
    n_comp = want[2].size
    assert np.array_equal(got.size[:n_comp], want[2]) and not got.size[n_comp:].any()
    assert np.array_equal(got.label, want[0]) and np.array_equal(got.cluster, want[1]) and np.array_equal(got.members, want[3])
    # the label alone, and the count alone
    got = ctx.components(edges, n_nodes, want=(), count=False)
    assert np.array_equal(got.label, want[0]) and got[1:] == (None, None, None, None)
    got = ctx.components(edges, n_nodes, want=())
    assert np.array_equal(got.label, want[0]) and got.n_components == n_comp


def test_host_and_device_memory(ctx, giant):
    import torch
    n_nodes, edges, want = giant
    d_edges = torch.from_numpy(edges.view(np.int32)).cuda()
    got = ctx.components(d_edges, n_nodes)
    for x in got[:4]:
        assert x.is_cuda and x.device == d_edges.device and x.dtype == torch.int32
    assert_same(got, want)
    got = ctx.components(d_edges, n_nodes, want=("cluster",), count=False)
    ctx.synchronize()
    assert got.size is None and got.members is None and np.array_equal(got.cluster.cpu().numpy().view(np.uint32), want[1])
    # an async_device context: the call with the count waits for it, the one without is ordered by the stream
    actx = lib.Context(0, async_device=True)
    try:
        assert_same(actx.components(d_edges, n_nodes), want)
        got = actx.components(d_edges, n_nodes, count=False)
        actx.synchronize()
        assert np.array_equal(got.label.cpu().numpy().view(np.uint32), want[0])
        assert np.array_equal(got.members.cpu().numpy().view(np.uint32), want[3])
    finally:
        actx.close()


# ---- skipped edges ---------------------------------------------------------------------------------------------------------------------
def test_skipped_edges(ctx):
    rng = np.random.default_rng(10)
    n = 3000
    valid = random_pairs(rng, n, 2500)
    valid = valid[valid[:, 0] != valid[:, 1]]
    want = reference_components(n, valid[:, 0], valid[:, 1])
    assert_shows_something(want)
    loops = pairs_of(np.arange(0, n, 7), np.arange(0, n, 7))
    out_of_range = np.array([[0, n], [n, 1], [2, n + 1], [n + 1, n], [3, 0xFFFFFFFF], [0xFFFFFFFF, 4], [0xFFFFFFFF, 0xFFFFFFFF],
                             [n - 1, n], [0x80000000, 5]], np.uint32)
    mixed = np.concatenate([valid, loops, valid[:500], valid[::3, ::-1], np.repeat(out_of_range, 40, axis=0)])
    mixed = np.ascontiguousarray(mixed[rng.permutation(mixed.shape[0])])
    assert_same(ctx.components(mixed, n), want)
    assert_same(ctx.components(valid, n), want)
    # nothing but edges that are skipped: every node is its own cluster
    alone = reference_components(n, [], [])
    assert_same(ctx.components(np.concatenate([loops, out_of_range]), n), alone)


# ---- records ------------------------------------------------------------------------------------------------------------------------
def bridged(rng, stride, weight_at, bridge_weight):
    """two components of 300 nodes each (edges of weight 1000) and one edge of weight `bridge_weight` between them; 50 nodes alone"""
    n_half, n = 300, 650
    rows = []
    for base in (0, n_half):
        chain = rng.permutation(n_half) + base
        rows.append(np.stack([chain[:-1], chain[1:]], axis=1))
        rows.append(rng.integers(base, base + n_half, (200, 2)))
    uv = np.concatenate(rows + [np.array([[n_half + 17, 42]])])
    rec = rng.integers(0, 1 << 32, (uv.shape[0], stride), dtype=np.uint64).astype(np.uint32)  # the other words hold anything
    rec[:, 0:2] = uv
    if weight_at:
        rec[:, weight_at] = 1000
        rec[-1, weight_at] = bridge_weight
    return n, np.ascontiguousarray(rec[rng.permutation(rec.shape[0])])


@pytest.mark.parametrize("stride,weight_at", [(3, 2), (8, 4), (8, 5)])
def test_records_with_a_weight(ctx, stride, weight_at):
    rng = np.random.default_rng(100 * stride + weight_at)
    n, rec = bridged(rng, stride, weight_at, 7)
    sizes = {}
    for min_weight in (6, 7, 8):
        sizes[min_weight] = check(ctx, n, rec, weight_at, min_weight).size.tolist()
    assert sizes[6][0] == sizes[7][0] == 600 and sizes[8][:2] == [300, 300]  # >= : the bridge counts at its own weight
    assert check(ctx, n, rec, 0, 8).size[0] == 600  # weight_at 0: min_weight is not looked at
    if stride == 8:  # the same records as a structured array, as anchor_overlaps returns them
        ovl = rec.reshape(-1).view(REC)
        assert ovl.shape == (rec.shape[0],)
        for min_weight in (7, 8):
            assert check(ctx, n, ovl, weight_at, min_weight).size.tolist() == sizes[min_weight]
    # a weight with its top bit set is unsigned
    n, rec = bridged(rng, stride, weight_at, 0x80000000)
    rec[:, weight_at] = np.where(rec[:, weight_at] == 1000, 0xFFFFFFF0, rec[:, weight_at])
    assert check(ctx, n, rec, weight_at, 0x80000000).size[0] == 600
    assert check(ctx, n, rec, weight_at, 0x80000001).size[:2].tolist() == [300, 300]


def test_pairs(ctx):
    rng = np.random.default_rng(11)
    n, rec = bridged(rng, 2, 0, 0)
    assert check(ctx, n, rec).size[0] == 600
    assert check(ctx, n, rec.view(np.int32)).size[0] == 600


# ---- neighbour lists ------------------------------------------------------------------------------------------------------------------
def knn_lists(rng, k):
    """two groups of 40 rows whose lists stay inside the group (eq 50 .. 59), one entry of eq 30 from row 3 to row 45, rows 80 .. 84
    with empty lists; lists shorter than k are filled with KNN_NONE / 0"""
    n, half = 85, 40
    idx = np.full((n, k), NONE, np.uint32)
    eq = np.zeros((n, k), np.uint16)
    for i in range(2 * half):
        base = (i // half) * half
        fill = int(rng.integers(1, k + 1)) if k > 1 else 1
        others = base + (i - base + 1 + rng.permutation(half - 1)[:fill]) % half  # never i itself
        others[0] = base + (i - base + 1) % half  # a ring: the group is connected whatever else is drawn
        idx[i, :others.size] = others
        eq[i, :others.size] = rng.integers(50, 60, others.size)
    idx[3, -1 if k > 1 else 0] = 45
    eq[3, -1 if k > 1 else 0] = 30
    return n, idx, eq


@pytest.mark.parametrize("k", [1, 5, 64])
def test_neighbour_lists(ctx, k):
    rng = np.random.default_rng(k)
    n, idx, eq = knn_lists(rng, k)
    assert k == 1 or (idx == NONE).any()
    sizes = {}
    for min_eq in (0, 29, 30, 31, 50, 60):
        want = reference_components(n, *reference_edges_of_knn(idx, eq, min_eq))
        if min_eq < 60:
            assert_shows_something(want)
        got = ctx.components_knn(idx, eq, min_eq)
        assert_same(got, want)
        sizes[min_eq] = got.size.tolist()
    if k > 1:  # (with k = 1 the bridge replaces the ring entry of row 3: the ring of group 0 opens, and stays one piece as a path)
        assert sizes[30][0] == 80 and sizes[31][:2] == [40, 40]
    assert sizes[29] == sizes[30] and sizes[60] == [1] * n
    # without eq every entry counts
    want = reference_components(n, *reference_edges_of_knn(idx, None, 0))
    assert_same(ctx.components_knn(idx, None), want)
    import torch
    d_idx, d_eq = torch.from_numpy(idx.view(np.int32)).cuda(), torch.from_numpy(eq.view(np.int16)).cuda()
    got = ctx.components_knn(d_idx, d_eq, 31)
    assert got.label.is_cuda
    assert_same(got, reference_components(n, *reference_edges_of_knn(idx, eq, 31)))


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_reads_to_clusters(ctx, oracle):
    """Three molecules of 2800 random bases, each tiled by five reads of 1200 that start 400 apart (one of them reverse-complemented),
    and one unrelated read; window 200, stride 100, strand-independent anchors.  Neighbouring reads share 800 bases cut into the same
    windows, so their overlap scores are far above 8, and random molecules share no 21-mer: the clusters are the molecules."""
    rng = np.random.default_rng(2026)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    reads, planted = [], []
    for mol in range(3):
        genome = bytes(rng.choice(acgt, size=2800))
        for j in range(5):
            r = genome[400 * j:400 * j + 1200]
            reads.append(revcomp(r) if (mol, j) == (1, 2) else r)
            planted.append(mol)
    reads.append(bytes(rng.choice(acgt, size=900)))
    planted.append(3)
    order = rng.permutation(len(reads))  # the reads of a molecule are not neighbours in the batch
    reads, planted = [reads[i] for i in order], np.array(planted)[order]
    bases, off = oracle.concat(reads)
    params = anchor.AnchorsGeneratorParameters("reads.fasta", 200, 16, 21, 100)
    hashes, _, _, row_off = ctx.read_anchors(bases, off, params.sketch_params(fhash=A.FHASH_CANON_VALUE), 200, 100, want_counts=False)
    kw = dict(n_keys=2, min_common=1, strands=2, band=1, min_score=8)
    ro = anchor.read_overlaps(ctx, hashes, row_off, params, **kw)
    want = reference_components(len(reads), ro[:, 0], ro[:, 1])
    assert_shows_something(want)
    cluster, sizes, members = anchor.read_clusters(ctx, hashes, row_off, params, want_members=True, first_readnum=100, **kw)
    assert cluster.dtype == np.int64 and np.array_equal(cluster, want[1]) and np.array_equal(sizes, want[2])
    assert np.array_equal(members, want[3].astype(np.int64) + 100)
    # the clusters are the molecules
    assert sorted(sizes.tolist()) == [1, 5, 5, 5]
    for mol in range(4):
        assert np.unique(cluster[planted == mol]).size == 1
    # by votes: the records whose band holds at least 4 matched windows
    all_ro = anchor.read_overlaps(ctx, hashes, row_off, params, **dict(kw, min_score=0))
    keep = all_ro[:, 5] >= 4
    want_v = reference_components(len(reads), all_ro[keep, 0], all_ro[keep, 1])
    cluster_v, sizes_v = anchor.read_clusters(ctx, hashes, row_off, params, by="votes", **dict(kw, min_score=4))
    assert np.array_equal(cluster_v, want_v[1]) and np.array_equal(sizes_v, want_v[2])
    # the same with the rows on the device
    import torch
    dh = torch.from_numpy(np.ascontiguousarray(hashes).view(np.int64)).cuda()
    d_cluster, d_sizes = anchor.read_clusters(ctx, dh, row_off, params, **kw)
    assert np.array_equal(d_cluster, cluster) and np.array_equal(d_sizes, sizes)


def genome_families():
    """three ancestors of 2000 random bases, twelve copies of each with 1 % of the bases substituted, shuffled"""
    from kmerutils_amd import synth
    rng = np.random.default_rng(77)
    genomes, family = [], []
    for f in range(3):
        ancestor = synth.ACGT[rng.integers(0, 4, 2000)]
        for _ in range(12):
            g = ancestor.copy()
            pos = np.flatnonzero(rng.random(g.size) < 0.01)
            g[pos] = synth.ACGT[(np.searchsorted(synth.ACGT, g[pos]) + rng.integers(1, 4, size=pos.size)) % 4]
            genomes.append(bytes(g))
            family.append(f)
    order = rng.permutation(len(genomes))
    return [genomes[i] for i in order], np.array(family)[order]


def test_signatures_to_clusters(ctx, oracle):
    """36 genomes in three families, ProbMinHash3a signatures (k = 8, m = 200), the 5 nearest neighbours of each, clustered at an
    identity of 0.5 (min_eq 100).  The oracle's signatures on the CPU give exactly the planted families at that threshold (asserted
    first); the device then has to give the oracle's lists, and their components."""
    from test_gpu_knn import knn_ref
    genomes, family = genome_families()
    m, k, threshold = 200, 5, 0.5
    p = A.SketchParams(A.ALGO_PROB3A, A.KMER32BIT, 8, m, A.SIG_U32, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)
    bases, off = oracle.concat(genomes)
    g = np.arange(len(genomes), dtype=np.uint32)
    widx, weq = knn_ref(oracle.sketch(bases, off, p), oracle.sketch(bases, off, p), k, g, g)
    assert S.min_eq_for_identity(threshold, m) == 100
    want = reference_components(len(genomes), *reference_edges_of_knn(widx, weq, 100))
    assert want[2].tolist() == [12, 12, 12], "the oracle does not give the planted families: change the mutation rate"
    for f in range(3):
        assert np.unique(want[1][family == f]).size == 1
    sig = np.asarray(S.SeqSketcher(8, m, ctx=ctx).sketch_probminhash3a(genomes, A.FHASH_CANON_INVHASH))
    idx, eq = ctx.sig_knn(sig, sig, k, g, g)
    assert np.array_equal(idx, widx) and np.array_equal(eq, weq)
    assert_same(S.neighbour_clusters(idx, eq, m, threshold, ctx=ctx), want)
    import torch
    d_sig = torch.from_numpy(sig.view(np.int32)).cuda()
    d_g = torch.from_numpy(g.view(np.int32)).cuda()
    d_idx, d_eq = ctx.sig_knn(d_sig, d_sig, k, d_g, d_g)
    assert_same(S.neighbour_clusters(d_idx, d_eq, m, threshold, ctx=ctx), want)
    # a threshold nothing reaches: 36 clusters of one
    assert S.neighbour_clusters(idx, eq, m, 1.0, ctx=ctx).size.tolist() == [1] * 36


# ---- status codes ----------------------------------------------------------------------------------------------------------------------
def p_(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


def raw(ctx, n_nodes, edges, n_edges, stride, weight_at, min_weight, label, mem=A.MEM_HOST, h=0, count=True):
    n = C.c_uint32(12345)
    rc = ctx.L.kmu_components(ctx.h if h == 0 else h, n_nodes, p_(edges), n_edges, stride, weight_at, min_weight, mem, p_(label), None, None,
                              None, C.byref(n) if count else None)
    return rc, int(n.value)


def raw_knn(ctx, n_nodes, idx, eq, k, min_eq, label, mem=A.MEM_HOST, h=0):
    n = C.c_uint32(12345)
    rc = ctx.L.kmu_components_knn(ctx.h if h == 0 else h, n_nodes, p_(idx), p_(eq), k, min_eq, mem, p_(label), None, None, None, C.byref(n))
    return rc, int(n.value)


def test_status_codes(ctx):
    edges = np.array([[0, 1, 9], [2, 3, 9], [3, 4, 1]], np.uint32)
    idx = np.array([[1], [0], [3], [2], [NONE]], np.uint32)
    eq = np.full((5, 1), 7, np.uint16)
    label = np.full(5, 77, np.uint32)
    bad, uns = A.E_BAD_ARG, A.E_UNSUPPORTED
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        # refused before anything is read or written
        assert raw(ctx, 5, edges, 3, 3, 2, 5, label, h=None)[0] == bad
        assert raw(ctx, 5, edges, 3, 3, 2, 5, None)[0] == bad
        assert raw(ctx, 5, None, 3, 3, 2, 5, label)[0] == bad
        assert raw(ctx, 5, edges, 3, 1, 0, 0, label)[0] == bad
        assert raw(ctx, 5, edges, 3, 0, 0, 0, label)[0] == bad
        assert raw(ctx, 5, edges, 3, 3, 1, 0, label)[0] == bad
        assert raw(ctx, 5, edges, 3, 3, 3, 0, label)[0] == bad
        assert raw(ctx, 5, edges, 3, 3, 2, 5, label, mem=7)[0] == bad
        assert raw(ctx, 0xFFFFFFFF, edges, 3, 3, 2, 5, label)[0] == uns
        assert raw_knn(ctx, 5, idx, eq, 1, 7, label, h=None)[0] == bad
        assert raw_knn(ctx, 5, idx, eq, 1, 7, None)[0] == bad
        assert raw_knn(ctx, 5, None, eq, 1, 7, label)[0] == bad
        assert raw_knn(ctx, 5, idx, eq, 0, 7, label)[0] == bad
        assert raw_knn(ctx, 5, idx, None, 1, 7, label)[0] == bad
        assert raw_knn(ctx, 5, idx, eq, 1, 7, label, mem=-1)[0] == bad
        assert raw_knn(ctx, 0xFFFFFFFF, idx, eq, 1, 7, label)[0] == uns
        with pytest.raises(lib.KmuError) as e:
            ctx.components(edges, 5, weight_at=1)
        assert e.value.code == bad
        # no nodes: 0 components, nothing written
        assert raw(ctx, 0, edges, 3, 3, 2, 5, label) == (A.OK, 0)
        assert raw_knn(ctx, 0, idx, eq, 0, 7, label) == (A.OK, 0)
        got = ctx.components(edges[:0], 0)
        assert got.n_components == 0 and all(x.shape == (0,) for x in got[:4])
        assert (label == 77).all()
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        # no edges: every node is its own cluster (the edge array may be missing); no hook runs
        assert raw(ctx, 5, None, 0, 2, 0, 0, label) == (A.OK, 5) and label.tolist() == [0, 1, 2, 3, 4]
        got = ctx.components(edges[:0], 5)
        assert got.label.tolist() == [0, 1, 2, 3, 4] == got.cluster.tolist() == got.members.tolist() and got.size.tolist() == [1] * 5
        assert "k_cc_init" in ctx.profile_get() and "k_cc_hook" not in ctx.profile_get()
        # the good calls, through the same raw path
        assert raw(ctx, 5, edges, 3, 3, 2, 5, label) == (A.OK, 3) and label.tolist() == [0, 0, 2, 2, 4]
        assert raw(ctx, 5, edges, 3, 3, 2, 1, label, count=False)[0] == A.OK and label.tolist() == [0, 0, 2, 2, 2]
        assert raw_knn(ctx, 5, idx, eq, 1, 7, label) == (A.OK, 3) and label.tolist() == [0, 0, 2, 2, 4]
        assert raw_knn(ctx, 5, idx, eq, 1, 8, label) == (A.OK, 5) and label.tolist() == [0, 1, 2, 3, 4]
        assert raw_knn(ctx, 5, idx, None, 1, 0, label) == (A.OK, 3)
        prof = ctx.profile_get()
        assert all(name in prof for name in ("k_cc_init", "k_cc_hook", "k_cc_flatten"))
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()

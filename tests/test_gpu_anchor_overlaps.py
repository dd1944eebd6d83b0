"""-m gpu: kmu_anchor_overlaps against reference_overlaps (tests/test_anchor_overlaps_abi.py: the rules of include/kmu.h over
dicts), whole record arrays compared exactly.  `pairs` / `dist` are built directly from (read, slice) coordinates, so the tests
control the entries, the runs (one diagonal of one read pair) and the read pairs; every case asserts that it expects a record.

Sizes: T = ANCHOR_SORT_TILE entries are ranked by one workgroup per radix pass and T window pairs are turned into entries by one
workgroup, a run is reduced 64 entries at a time, and the device scans (over the per-entry flags) change kernels above 32768."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib
from test_anchor_overlaps_abi import REC, reference_overlaps

pytestmark = pytest.mark.gpu
T = A.ANCHOR_SORT_TILE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def layout(rows_per_read):
    return np.concatenate([[0], np.cumsum(np.asarray(rows_per_read, np.uint64))]).astype(np.uint64)


def mk_pairs(off_q, off_db, ra, sa, rb, sb):
    """window pairs (row a, row b) from (read, slice) of both sides"""
    ra, sa, rb, sb = (np.asarray(x).astype(np.int64) for x in (ra, sa, rb, sb))
    a, b = off_q.astype(np.int64)[ra] + sa, off_db.astype(np.int64)[rb] + sb
    assert (a < off_q.astype(np.int64)[ra + 1]).all() and (b < off_db.astype(np.int64)[rb + 1]).all() and (sa >= 0).all() and (sb >= 0).all()
    return np.ascontiguousarray(np.stack([a, b], axis=1).astype(np.uint32))


def mk_dist(rng, n, lo=0, hi=6):
    d = np.zeros((n, 3), np.uint32)
    d[:, 0] = rng.integers(lo, hi, n)
    d[:, 1:] = 16
    return d


def check(ctx, pairs, dist, off_q, off_db=None, strands=2, band=1, min_score=1, upper=False):
    want = reference_overlaps(pairs, dist, off_q, off_db, strands, band, min_score, upper)
    assert want.shape[0] > 0, "the case expects no record: it would show nothing"
    got = ctx.anchor_overlaps(pairs, dist, off_q, off_db, strands=strands, band=band, min_score=min_score, upper=upper)
    assert got.dtype == REC and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "records %s differ; first: got %s, want %s" % (bad[:8].tolist(), got[bad[0]], want[bad[0]])
    return got


def random_case(rng, n_pairs, n_reads=12, rows=30):
    off = layout(np.full(n_reads, rows))
    pairs = mk_pairs(off, off, rng.integers(0, n_reads, n_pairs), rng.integers(0, rows, n_pairs), rng.integers(0, n_reads, n_pairs),
                     rng.integers(0, rows, n_pairs))
    return off, pairs, mk_dist(rng, n_pairs)


# ---- the sort tile ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strands,n_pairs", [(1, T - 1), (1, T), (1, T + 1), (1, 2 * T + 1), (2, T // 2), (2, T // 2 + 1), (2, T + 1)])
def test_entry_counts_around_the_sort_tile(ctx, strands, n_pairs):
    rng = np.random.default_rng(10 * n_pairs + strands)
    off, pairs, dist = random_case(rng, n_pairs)  # drawn at random: the input is in no order
    check(ctx, pairs, dist, off, strands=strands, band=1)
    check(ctx, pairs, None, off, strands=strands, band=0, upper=True)


# ---- run shapes ---------------------------------------------------------------------------------------------------------------
def runs_case(lengths, gap=2):
    """one read pair, one strand; run k has lengths[k] entries on diagonal k * gap, in sorted order one after the other"""
    rows = 2 * max(lengths) + gap * len(lengths) + 8
    off = layout([rows, rows])
    sa, sb = [], []
    for k, n in enumerate(lengths):
        d = k * gap
        sa.append(d + np.arange(n))  # slice_a - slice_b = d
        sb.append(np.arange(n))
    sa, sb = np.concatenate(sa), np.concatenate(sb)
    return off, mk_pairs(off, off, np.zeros(sa.size, int), sa, np.ones(sa.size, int), sb)


def test_runs_that_end_around_a_chunk_and_a_tile(ctx):
    # ends at 63, 64, 65 | 128, 193, 256 | ... T - 1, T, T + 1
    lengths = [63, 1, 1, 63, 65, 63, T - 1 - 256, 1, 1, 70]
    assert np.cumsum(lengths).tolist()[:3] == [63, 64, 65] and np.cumsum(lengths).tolist()[6:9] == [T - 1, T, T + 1]
    off, pairs = runs_case(lengths)
    rng = np.random.default_rng(3)
    dist = mk_dist(rng, pairs.shape[0], 1, 4)
    for band in (0, 1, 2):
        for shuffled in (pairs, pairs[rng.permutation(pairs.shape[0])]):
            got = check(ctx, shuffled, None, off, strands=1, band=band)
            assert got["votes"][0] == (T - 1 - 256 if band < 2 else T - 1 - 256 + 63)  # band 2 reaches the run in front
    perm = rng.permutation(pairs.shape[0])
    check(ctx, pairs[perm], dist[perm], off, strands=1, band=0)
    # the same runs, each the only one of a read pair of its own: the read pair changes where the run does
    off10 = layout(np.full(11, int(off[1])))
    ra = np.repeat(np.arange(len(lengths)), lengths)
    own = mk_pairs(off10, off10, ra, pairs[:, 0].astype(np.int64) - 2 * ra, np.full(ra.size, 10), pairs[:, 1].astype(np.int64) - int(off[1]))
    got = check(ctx, own[perm], dist[perm], off10, strands=1, band=1, min_score=0)
    assert got["votes"].tolist() == lengths and (got["diag"] == 0).all()


def test_one_run_of_three_tiles(ctx):
    off, pairs = runs_case([3 * T])
    rng = np.random.default_rng(4)
    dist = mk_dist(rng, 3 * T, 0, 1000)
    got = check(ctx, pairs[rng.permutation(3 * T)], None, off, strands=1, band=0)
    assert got.tolist() == [(0, 1, 0, 0, 3 * T, 3 * T, 0, 3 * T - 1)]
    got = check(ctx, pairs, dist, off, strands=1, band=8)
    assert got["score"][0] == dist[:, 0].sum() and got["votes"][0] == 3 * T


def test_five_thousand_runs_of_one_entry(ctx):
    off, pairs = runs_case([1] * 5000, gap=3)
    rng = np.random.default_rng(5)
    dist = mk_dist(rng, 5000, 1, 50)
    perm = rng.permutation(5000)
    for band in (0, 2, 3, 8):
        check(ctx, pairs[perm], dist[perm], off, strands=1, band=band)
    # ... and as 5000 read pairs
    offn = layout(np.full(5001, 4))
    own = mk_pairs(offn, offn, np.arange(5000), rng.integers(0, 4, 5000), np.full(5000, 5000), rng.integers(0, 4, 5000))
    got = check(ctx, own[perm], dist[perm], offn, strands=2, band=1)
    assert got.shape[0] == 5000


# ---- every radix pass of both sorts ---------------------------------------------------------------------------------------------
def test_every_radix_pass_matters(ctx):
    """read ids that differ only in one byte each (up to 2^24 + 2: most reads have no row), and diagonals whose biased value
    d + 2^31 differs in one byte each"""
    ids = [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, (1 << 24) + 2]
    n_reads = (1 << 24) + 3
    big = 1 << 25  # rows of the reads that carry the diagonals
    rows = np.zeros(n_reads, np.uint64)
    rows[ids] = 8
    rows[[0, 1 << 24]] = big
    off = layout(rows)
    assert int(off[-1]) < 1 << 31
    rng = np.random.default_rng(6)
    # every ordered pair of the ids, on a few small diagonals
    ra, rb = (x.ravel() for x in np.meshgrid(ids, ids, indexing="ij"))
    ra, rb = np.repeat(ra, 3), np.repeat(rb, 3)
    sa, sb = rng.integers(0, 8, ra.size), rng.integers(0, 8, ra.size)
    # reads 0 and 2^24: slice_a - slice_b = +-1, +-256, +-65536, +-2^24, 0 and slice_a + slice_b = the same sums with slice_b = 0 or 1
    steps = [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24]
    dsa = np.array(steps + [0] * len(steps) + [s + 1 for s in steps])
    dsb = np.array([0] * len(steps) + steps + [1] * len(steps))
    pairs = np.concatenate([mk_pairs(off, off, ra, sa, rb, sb),
                            mk_pairs(off, off, np.zeros(dsa.size, int), dsa, np.full(dsa.size, 1 << 24), dsb),
                            mk_pairs(off, off, np.full(dsa.size, 1 << 24), dsb, np.zeros(dsa.size, int), dsa)])
    pairs = pairs[rng.permutation(pairs.shape[0])]
    dist = mk_dist(rng, pairs.shape[0], 1, 9)
    for strands, band in ((1, 0), (2, 0), (2, 1)):
        got = check(ctx, pairs, dist, off, strands=strands, band=band)
        assert got.shape[0] == len(ids) ** 2
    # band 0, one strand, every pair weighing 1 and min_score 0: all diagonals of (0, 2^24) tie, the smallest (-2^24) wins
    got = check(ctx, pairs, None, off, strands=1, band=0, min_score=0)
    r = got[(got["read_a"] == 0) & (got["read_b"] == 1 << 24)]
    assert r["diag"].tolist() == [-(1 << 24)] or r["score"][0] > 1


# ---- negative diagonals, large sums ---------------------------------------------------------------------------------------------
def test_negative_diagonals_and_large_sums(ctx):
    off = layout([5, 70_001, 70_001])
    rng = np.random.default_rng(7)
    sb = np.concatenate([[70_000, 70_000, 69_999, 65_536, 65_535, 1, 0], rng.integers(0, 70_001, 200)])
    pairs = np.concatenate([mk_pairs(off, off, np.zeros(sb.size, int), np.zeros(sb.size, int), np.ones(sb.size, int), sb),
                            mk_pairs(off, off, [2, 2, 2, 2], [70_000, 69_999, 69_998, 5], [1, 1, 1, 1], [69_998, 69_999, 70_000, 3])])
    got = check(ctx, pairs, None, off, strands=1, band=1)
    assert got.tolist()[0] == (0, 1, 0, -70_000, 3, 3, 0, 0)
    got = check(ctx, pairs, None, off, strands=2, band=0)
    assert got.tolist()[0] == (0, 1, 0, -70_000, 2, 2, 0, 0)  # strand 1 has the same runs at +70 000: the tie goes to strand 0
    assert got.tolist()[1] == (2, 1, 1, 139_998, 3, 3, 69_998, 70_000)  # three sums of 139 998 against differences of 2, 0, -2
    check(ctx, pairs[:, ::-1].copy(), None, off, strands=2, band=1)


# ---- bands ----------------------------------------------------------------------------------------------------------------------
def band_case(rng):
    """one read pair whose occupied diagonals lie 1, 2, .. 10 apart, twice over; some on a second read pair behind it"""
    d = np.cumsum(np.concatenate([[0], np.arange(1, 11), np.arange(10, 0, -1)]))
    off = layout([200, 200, 200])
    reps = rng.integers(1, 4, d.size)
    dd = np.repeat(d, reps)
    sb = rng.integers(0, 60, dd.size)
    pairs = np.concatenate([mk_pairs(off, off, np.zeros(dd.size, int), dd + sb, np.ones(dd.size, int), sb),
                            mk_pairs(off, off, np.zeros(dd.size, int), dd + sb, np.full(dd.size, 2), sb)[::3]])
    perm = rng.permutation(pairs.shape[0])
    return off, pairs[perm], mk_dist(rng, pairs.shape[0], 1, 4)[perm]


@pytest.mark.parametrize("band", range(A.OVL_MAX_BAND + 1))
def test_every_band_width(ctx, band):
    off, pairs, dist = band_case(np.random.default_rng(8))
    check(ctx, pairs, dist, off, strands=1, band=band)
    check(ctx, pairs, dist, off, strands=2, band=band)
    check(ctx, pairs, None, off, strands=1, band=band)


@pytest.mark.parametrize("band", [1, 8])
def test_a_band_stops_at_the_strand_and_at_the_read_pair(ctx, band):
    off = layout([40, 40, 40])
    # (0, 1): slice_b = 0, so both strands have the same diagonals 3 and 5: the last run of strand 0 (d = 5) is followed by the
    # first of strand 1 (d = 3, 5); a look-ahead that only compared diagonals would add them
    # (0, 2): diagonal 6 and 7 right behind (0, 1)'s last run (strand 1, d = 5)
    pairs = np.concatenate([mk_pairs(off, off, [0, 0, 0], [3, 5, 5], [1, 1, 1], [0, 0, 0]),
                            mk_pairs(off, off, [0, 0], [6, 7], [2, 2], [0, 0])])
    dist = np.array([[1, 9, 9], [2, 9, 9], [2, 9, 9], [100, 9, 9], [100, 9, 9]], np.uint32)
    got = check(ctx, pairs, dist, off, strands=2, band=band)
    assert got.tolist() == [(0, 1, 0, 3 if band >= 2 else 5, 5 if band >= 2 else 4, 3 if band >= 2 else 2, 3 if band >= 2 else 5, 5),
                            (0, 2, 0, 6, 200, 2, 6, 7)]
    got = check(ctx, pairs, dist, off, strands=1, band=band)
    assert got["score"].tolist() == [5 if band >= 2 else 4, 200]


# ---- ties, weights, the clamp, the filter -----------------------------------------------------------------------------------------
def test_ties(ctx):
    off = layout([10, 10, 10, 10])
    # (0, 1): the hand case of the reference's own test -- strand 0 from d = 1 and strand 1 at d = 3 tie at 2 under band 2
    pairs = np.array([[2, 11], [3, 10]], np.uint32)
    assert check(ctx, pairs, None, off, strands=2, band=2).tolist() == [(0, 1, 0, 1, 2, 2, 2, 3)]
    assert check(ctx, pairs, None, off, strands=2, band=1).tolist() == [(0, 1, 1, 3, 2, 2, 2, 3)]
    assert check(ctx, pairs, None, off, strands=1, band=0).tolist() == [(0, 1, 0, 1, 1, 1, 2, 2)]
    # two diagonals with equal scores: the smaller d, wherever its entries stand in the input
    pairs = mk_pairs(off, off, [2, 2, 2, 2], [9, 8, 3, 4], [3, 3, 3, 3], [2, 1, 7, 8])  # d = 7, 7, -4, -4
    for order in ([0, 1, 2, 3], [3, 1, 2, 0]):
        assert check(ctx, pairs[order], None, off, strands=1, band=0).tolist() == [(2, 3, 0, -4, 2, 2, 3, 4)]
    # weights decide otherwise
    dist = np.array([[3, 9, 9], [3, 9, 9], [1, 9, 9], [4, 9, 9]], np.uint32)
    assert check(ctx, pairs, dist, off, strands=1, band=0).tolist() == [(2, 3, 0, 7, 6, 2, 8, 9)]
    dist[:, 0] = [2, 3, 1, 4]  # 5 : 5 again
    assert check(ctx, pairs, dist, off, strands=1, band=0).tolist() == [(2, 3, 0, -4, 5, 2, 3, 4)]
    dist[:, 0] = 0  # weights of 0 (min_common = 0 lets them through): a record with score 0 when min_score is 0
    assert check(ctx, pairs, dist, off, strands=1, band=0, min_score=0).tolist() == [(2, 3, 0, -4, 0, 2, 3, 4)]
    assert ctx.anchor_overlaps(pairs, dist, off, strands=1, band=0, min_score=1).shape == (0,)


def test_score_clamp(ctx):
    off = layout([10, 10])
    w = (1 << 32) // 3 + 1
    pairs = mk_pairs(off, off, [0, 0, 0, 0], [1, 2, 3, 9], [1, 1, 1, 1], [0, 1, 2, 0])
    dist = np.array([[w, 1, 1], [w, 1, 1], [w, 1, 1], [0xFFFFFFFF, 1, 1]], np.uint32)
    assert 3 * w > 0xFFFFFFFF
    # d = 1 holds 3 w > 2^32 - 1 >= the weight on d = 9: the unclamped sum decides, the record shows the clamp
    assert check(ctx, pairs, dist, off, strands=1, band=0).tolist() == [(0, 1, 0, 1, 0xFFFFFFFF, 3, 1, 3)]
    assert check(ctx, pairs, dist, off, strands=1, band=0, min_score=0xFFFFFFFF).shape[0] == 1
    assert check(ctx, pairs[:2], dist[:2], off, strands=1, band=0).tolist() == [(0, 1, 0, 1, 2 * w, 2, 1, 2)]


def test_min_score_filter(ctx):
    rng = np.random.default_rng(12)
    off, pairs, dist = random_case(rng, 600, n_reads=20, rows=12)
    every = check(ctx, pairs, dist, off, strands=2, band=1, min_score=0)
    assert check(ctx, pairs, dist, off, strands=2, band=1, min_score=1).shape[0] <= every.shape[0]
    median = int(np.median(every["score"]))
    half = check(ctx, pairs, dist, off, strands=2, band=1, min_score=median)
    assert every.shape[0] // 4 < half.shape[0] < every.shape[0] and (half["score"] >= median).all()


# ---- KMU_OVL_UPPER, the order of the input -------------------------------------------------------------------------------------------
def test_upper(ctx):
    off = layout([10, 10, 10])
    # (0, 2), (2, 0), (2, 2), (1, 1), (1, 2), (2, 1)
    pairs = mk_pairs(off, off, [0, 2, 2, 1, 1, 2, 0], [1, 4, 5, 5, 6, 2, 2], [2, 0, 2, 1, 2, 1, 2], [4, 1, 5, 5, 2, 6, 5])
    both = check(ctx, pairs, None, off, strands=2, band=1)
    assert [(r[0], r[1]) for r in both.tolist()] == [(0, 2), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]
    up = check(ctx, pairs, None, off, strands=2, band=1, upper=True)
    assert up.tolist() == [r for r in both.tolist() if r[0] < r[1]] and up.shape[0] == 2
    # a tile of pairs where some survive and a tile where none does: the compaction across tiles
    rng = np.random.default_rng(13)
    n = 2 * T + 77
    ra, rb = rng.integers(0, 3, n), rng.integers(0, 3, n)
    ra[T:2 * T], rb[T:2 * T] = 2, 1
    pairs = mk_pairs(off, off, ra, rng.integers(0, 10, n), rb, rng.integers(0, 10, n))
    dist = mk_dist(rng, n)
    assert check(ctx, pairs, dist, off, strands=2, band=1, upper=True).shape[0] == 3
    check(ctx, pairs, dist, off, strands=1, band=0, upper=True)
    # two different sides: read ids of the two sides are compared as numbers
    off_db = layout([7, 7, 7, 7])
    pairs = mk_pairs(off, off_db, [0, 1, 2, 2], [1, 1, 1, 2], [0, 3, 2, 3], [1, 2, 3, 4])
    assert [(r[0], r[1]) for r in check(ctx, pairs, None, off, off_db, strands=1, upper=True).tolist()] == [(1, 3), (2, 3)]


def test_the_order_of_the_input_does_not_matter(ctx):
    rng = np.random.default_rng(14)
    off, pairs, dist = random_case(rng, 3000, n_reads=6, rows=25)
    first = check(ctx, pairs, dist, off, strands=2, band=1)
    for _ in range(2):
        perm = rng.permutation(3000)
        again = ctx.anchor_overlaps(np.ascontiguousarray(pairs[perm]), np.ascontiguousarray(dist[perm]), off, strands=2, band=1)
        assert again.tobytes() == first.tobytes()
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    assert ctx.anchor_overlaps(np.ascontiguousarray(pairs[order]), np.ascontiguousarray(dist[order]), off, strands=2,
                               band=1).tobytes() == first.tobytes()


# ---- the scans --------------------------------------------------------------------------------------------------------------------
def test_scans_above_their_single_block_size(ctx):
    """40 000 window pairs, one strand, each a read pair of its own: 40 000 runs, read pairs and records, all above 32 768; and 40
    tiles of pairs under KMU_OVL_UPPER"""
    rng = np.random.default_rng(15)
    n_reads = 300
    off = layout(np.full(n_reads, 3))
    rp = rng.permutation(n_reads * n_reads)[:40_000]
    pairs = mk_pairs(off, off, rp // n_reads, rng.integers(0, 3, rp.size), rp % n_reads, rng.integers(0, 3, rp.size))
    dist = mk_dist(rng, rp.size, 1, 5)
    got = check(ctx, pairs, dist, off, strands=1, band=1)
    assert got.shape[0] == 40_000
    got = check(ctx, pairs, dist, off, strands=2, band=1, min_score=3, upper=True)
    assert 1000 < got.shape[0] < 20_000


# ---- capacity, memory mode, argument errors -----------------------------------------------------------------------------------------
def raw(ctx, pairs, dist, n_pairs, off_q, nq, off_db, ndb, strands, band, min_score, flags, out, cap, h=None, mem=A.MEM_HOST):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_uint64(12345)
    rc = ctx.L.kmu_anchor_overlaps(ctx.h if h is None else h, p(pairs), p(dist), n_pairs, p(off_q), nq, p(off_db), ndb, strands, band,
                                   min_score, flags, mem, p(out), cap, C.byref(n))
    return rc, int(n.value)


@pytest.fixture(scope="module")
def batch():
    rng = np.random.default_rng(16)
    return random_case(rng, 500, n_reads=9, rows=14)


def test_count_only_call_and_capacity(ctx, batch):
    off, pairs, dist = batch
    want = reference_overlaps(pairs, dist, off, None, 2, 1, 2, False)
    total = want.shape[0]
    assert total > 2
    args = (pairs, dist, 500, off, 9, off, 9, 2, 1, 2, 0)
    assert raw(ctx, *args, None, 0) == (A.OK, total)
    out = np.zeros(total, REC)
    assert raw(ctx, *args, out, total - 1) == (A.E_BAD_ARG, total)
    assert raw(ctx, *args, out, total) == (A.OK, total)
    assert np.array_equal(out, want)
    out2 = np.zeros(total + 5, REC)  # more room than needed
    assert raw(ctx, *args, out2, total + 5) == (A.OK, total)
    assert np.array_equal(out2[:total], want) and out2[total:].tobytes() == bytes(5 * 32)


def test_device_tensors_give_the_same_bytes(ctx, batch):
    import torch
    off, pairs, dist = batch
    dp, dd = torch.from_numpy(pairs.view(np.int32)).cuda(), torch.from_numpy(dist.view(np.int32)).cuda()
    doff = torch.from_numpy(off.view(np.int64)).cuda()
    for kw in (dict(strands=2, band=1, min_score=2), dict(strands=1, band=0, upper=True), dict(strands=2, band=8, min_score=0)):
        want = ctx.anchor_overlaps(pairs, dist, off, **kw)
        assert want.shape[0] > 0 and np.array_equal(want, reference_overlaps(pairs, dist, off, **kw))
        got = ctx.anchor_overlaps(dp, dd, doff, **kw)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (want.shape[0], 8)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        got = ctx.anchor_overlaps(dp, None, off, **kw)  # host offsets are copied up; no weights
        assert got.cpu().numpy().tobytes() == ctx.anchor_overlaps(pairs, None, off, **kw).tobytes()
    # offsets that the diagonal field cannot hold, read on the device: refused at the end of the call
    long_off = torch.from_numpy(np.array([0, 1 << 31], np.uint64).view(np.int64)).cuda()
    with pytest.raises(lib.KmuError) as e:
        ctx.anchor_overlaps(dp, dd, long_off, strands=1)
    assert e.value.code == A.E_UNSUPPORTED


def test_empty_input_and_argument_errors_launch_nothing(ctx, batch):
    off, pairs, dist = batch
    out = np.zeros(4, REC)
    ok = (pairs, dist, 500, off, 9, off, 9, 2, 1, 1, 0, out, 4)

    def with_(**kw):
        names = ["pairs", "dist", "n_pairs", "off_q", "nq", "off_db", "ndb", "strands", "band", "min_score", "flags", "out", "cap"]
        a = dict(zip(names, ok))
        a.update(kw)
        return raw(ctx, *[a[n] for n in names])
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        assert with_(n_pairs=0) == (A.OK, 0)
        assert ctx.anchor_overlaps(pairs[:0], None, off).shape == (0,)
        bad, uns = A.E_BAD_ARG, A.E_UNSUPPORTED
        assert with_(pairs=None)[0] == bad
        assert with_(off_q=None)[0] == bad
        assert with_(off_db=None)[0] == bad
        assert with_(strands=0)[0] == bad
        assert with_(strands=3)[0] == bad
        assert with_(flags=2)[0] == bad
        assert with_(flags=A.OVL_UPPER | 0x80000000)[0] == bad
        L = lib.load()
        n = C.c_uint64(0)
        pp, po = pairs.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p)
        assert L.kmu_anchor_overlaps(None, pp, None, 500, po, 9, po, 9, 2, 1, 1, 0, A.MEM_HOST, None, 0, C.byref(n)) == bad
        assert L.kmu_anchor_overlaps(ctx.h, pp, None, 500, po, 9, po, 9, 2, 1, 1, 0, A.MEM_HOST, None, 0, None) == bad
        # unsupported sizes are refused before any pair is read: the arrays may be short
        assert with_(band=A.OVL_MAX_BAND + 1)[0] == uns
        assert with_(n_pairs=1 << 32, strands=1)[0] == uns
        assert with_(n_pairs=1 << 31, strands=2)[0] == uns
        assert with_(n_pairs=(1 << 32) - 1, strands=2)[0] == uns
        long_off = np.array([0, 5, 1 << 31], np.uint64)
        assert with_(off_q=long_off, nq=2, strands=1)[0] == uns
        assert with_(off_db=long_off, ndb=2, strands=1)[0] == uns
        half = np.array([0, (1 << 30) + 1], np.uint64)  # each fits, their sum of slices does not fit an int32
        assert with_(off_q=half, nq=1, off_db=half, ndb=1, strands=2)[0] == uns
        with pytest.raises(lib.KmuError) as e:
            ctx.anchor_overlaps(pairs, dist, off, band=9)
        assert e.value.code == uns
        assert (out == np.zeros(4, REC)).all()
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        check(ctx, pairs, dist, off)
        assert "k_ovl_best_write" in ctx.profile_get()
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def revcomp(s):
    return s.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def test_reads_to_overlaps(ctx, oracle):
    """Six reads cut from one random genome at known starts, window 200, stride 100, strand-independent anchors.  Read 3 is the
    reverse complement of genome[600:2000]; reads 0 and 1 start 3 strides apart; read 5 is unrelated.  (Checked on the CPU
    with the oracle's bottom-k rows and a join in Python: the same pairs, the same records.)"""
    rng = np.random.default_rng(2025)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = bytes(rng.choice(acgt, size=4000))
    starts = [0, 300, 1000, 600, 2200]
    reads = [genome[0:1600], genome[300:1900], genome[1000:2600], revcomp(genome[600:2000]), genome[2200:3800],
             bytes(rng.choice(acgt, size=900))]
    bases, off = oracle.concat(reads)
    params = anchor.AnchorsGeneratorParameters("reads.fasta", 200, 16, 21, 100)
    sp = params.sketch_params(fhash=A.FHASH_CANON_VALUE)
    hashes, _, n, row_off = ctx.read_anchors(bases, off, sp, 200, 100, want_counts=False)
    group = np.repeat(np.arange(len(reads), dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    pairs, dist = ctx.anchor_match(hashes, hashes, n_keys=2, min_common=1, group_q=group, group_db=group)
    assert pairs.shape[0] > 20
    got = check(ctx, pairs, dist, row_off, strands=2, band=1)
    check(ctx, pairs, dist, row_off, strands=2, band=1, min_score=8, upper=True)
    rec = {(r[0], r[1]): r for r in got.tolist()}
    # same strand, starts 3 strides apart: slice s of read 1 is slice s + 3 of read 0
    assert rec[(0, 1)][2] == 0 and abs(rec[(0, 1)][3] - 3) <= 1 and rec[(1, 0)][2] == 0 and abs(rec[(1, 0)][3] + 3) <= 1
    assert rec[(1, 2)][2] == 0 and abs(rec[(1, 2)][3] - 7) <= 1
    # the reverse-complemented read: the opposite strand, against every read it overlaps and in both directions
    for other in (0, 1, 2):
        assert rec[(other, 3)][2] == 1 and rec[(3, other)][2] == 1
    # genome[600:2000] reversed: its slice t covers genome 2000 - 100 t - 200 .. 2000 - 100 t; slice s of read 0 covers 100 s ..:
    # s + t is about (2000 - 200) / 100 = 18
    assert abs(rec[(0, 3)][3] - 18) <= 1
    assert not any(5 in k for k in rec if rec[k][4] >= 8)
    # the Python layer: each read pair once, in bases, read numbers from first_readnum; the same with the rows on the device
    ro = anchor.read_overlaps(ctx, hashes, row_off, params, n_keys=2, min_common=1, strands=2, band=1, min_score=8, first_readnum=10)
    want = reference_overlaps(pairs, dist, row_off, None, 2, 1, 8, True)
    assert ro.shape == (want.shape[0], 8) and want.shape[0] >= 4
    assert ro[:, 0].tolist() == (want["read_a"] + 10).tolist() and ro[:, 1].tolist() == (want["read_b"] + 10).tolist()
    assert ro[:, 2].tolist() == want["strand"].tolist() and ro[:, 3].tolist() == (want["diag"].astype(np.int64) * 100).tolist()
    assert ro[:, 4].tolist() == want["score"].tolist() and ro[:, 5].tolist() == want["votes"].tolist()
    assert ro[:, 6].tolist() == (want["slice_a_min"].astype(np.int64) * 100).tolist()
    import torch
    dh = torch.from_numpy(np.ascontiguousarray(hashes).view(np.int64)).cuda()
    assert np.array_equal(anchor.read_overlaps(ctx, dh, row_off, params, n_keys=2, min_common=1, min_score=8, first_readnum=10), ro)
    assert starts[1] - starts[0] == 3 * params.get_stride()

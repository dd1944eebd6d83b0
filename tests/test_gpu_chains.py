"""-m gpu: kmu_seed_chains against `reference_chains` (tests/test_chains_abi.py: the contract of include/kmu.h in plain Python).
Every case compares whole record arrays exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_anchor_overlaps_abi import reference_overlaps  # noqa: E402
from test_chains_abi import Side, one_pair, reference_chains, side  # noqa: E402
from test_gpu_anchor_overlaps import random_case  # noqa: E402
from test_gpu_minimizers import expected, rand_reads, reference_hits, revcomp  # noqa: E402

pytestmark = pytest.mark.gpu
REC = np.dtype(A.CHAIN_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def check(ctx, pairs, q, db, span, max_gap, band, **kw):
    """the device's records, equal to the reference's in every byte"""
    want = reference_chains(pairs, q, db, span, max_gap, band, **kw)
    got = ctx.seed_chains(np.ascontiguousarray(pairs, np.uint32), q, db, span, max_gap, band, **kw)
    assert got.dtype == REC
    assert got.shape == want.shape, "%d records, want %d" % (got.shape[0], want.shape[0])
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "record %d: got %s, want %s" % (bad[0], got[bad[0]], want[bad[0]])
    return got


def from_groups(groups, n_reads):
    """groups: (read_a, read_b, strand, x array, pos_b array); every anchor gets a q entry and a db entry of its own"""
    ra = np.concatenate([np.full(len(g[3]), g[0]) for g in groups])
    rb = np.concatenate([np.full(len(g[3]), g[1]) for g in groups])
    s = np.concatenate([np.full(len(g[3]), g[2]) for g in groups])
    x = np.concatenate([np.asarray(g[3]) for g in groups])
    pb = np.concatenate([np.asarray(g[4]) for g in groups])
    n = x.size
    pairs = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)
    return pairs, side(x, ra, np.zeros(n, np.uint8), n_reads), side(pb, rb, s, n_reads)


def noisy_diagonal(rng, n, strand, step=30, noise=3):
    """n anchors along one diagonal: steps of 1 .. step in x, the same in b up to +-noise; on strand 1 b runs backwards"""
    x = np.cumsum(rng.integers(1, step + 1, n))
    y = x + 500 + rng.integers(-noise, noise + 1, n)
    return x, (y if strand == 0 else int(y.max()) + 7 - y)


# ---- the DP across chunks of 64 anchors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129, 200])
def test_group_sizes(ctx, n):
    rng = np.random.default_rng(n)
    for strand in (0, 1):
        x, pb = noisy_diagonal(rng, n, strand)
        pairs, q, db = from_groups([(0, 1, strand, x, pb)], 2)
        pairs = pairs[rng.permutation(n)]
        got = check(ctx, pairs, q, db, 15, 40, 8)
        assert got.shape == (1,) and got["n_anchors"][0] == n and got["strand"][0] == strand
        assert got["n_seeds"][0] > n // 2  # a chain, not fragments: the case exercises the carry across chunks
        check(ctx, pairs, q, db, 15, 12, 2)  # fragments: many fresh starts, equal scores


def lookback_group(n_fill):
    """anchor 0 at (0, 0), n_fill anchors that chain with nothing (b falls while x grows), then (100, 100)"""
    xf = 1 + np.arange(n_fill) % 90
    xf.sort()
    yf = 100000 - 10 * np.arange(n_fill)
    return from_groups([(0, 1, 0, np.concatenate([[0], xf, [100]]), np.concatenate([[0], yf, [100]]))], 2)


def test_lookback_edge(ctx):
    pairs, q, db = lookback_group(63)  # the predecessor sits exactly 64 back
    got = check(ctx, pairs, q, db, 15, 200000, 200000)
    assert got.tolist() == [(0, 1, 0, 30, 2, 65, 0, 115, 0, 115)]
    pairs, q, db = lookback_group(64)  # 65 back: out of sight, every anchor is alone and the first one wins
    got = check(ctx, pairs, q, db, 15, 200000, 200000)
    assert got.tolist() == [(0, 1, 0, 15, 1, 66, 0, 15, 0, 15)]


def test_gap_and_band_edges(ctx):
    max_gap, band = 100, 32
    steps = [(100, 100), (101, 101), (100, 101), (101, 100), (50, 82), (50, 83), (82, 50), (83, 50), (1, 1), (1, 2), (2, 1),
             (20, 28), (20, 27), (40, 56), (40, 55), (60, 92), (60, 91), (20, 21), (20, 22), (20, 24), (20, 23)]
    groups = []
    for r, (dx, dy) in enumerate(steps):
        for strand in (0, 1):
            groups.append((r, r + 1, strand, [7, 7 + dx], [900, 900 + dy] if strand == 0 else [900, 900 - dy]))
    pairs, q, db = from_groups(groups, len(steps) + 1)
    for span in (15, 1, 64):
        got = check(ctx, pairs, q, db, span, max_gap, band)
        assert got.shape == (len(steps),)
        if span == 15:
            assert got["n_seeds"].tolist() == [2, 1, 1, 1, 2, 1, 2, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2]
            assert got["score"][[8, 11, 12, 13, 14]].tolist() == [16, 15 + 15 - 1, 15 + 15 - 1, 15 + 15 - 3, 15 + 15 - 2]


@pytest.mark.parametrize("span,max_gap,band", [(3, 4, 2), (2, 7, 7), (64, 3, 0)])
def test_ties_everywhere(ctx, span, max_gap, band):
    rng = np.random.default_rng(span)
    nq, ndb = 60, 50
    q = side(rng.integers(0, 8, nq), rng.integers(0, 4, nq), rng.integers(0, 2, nq), 4)
    db = side(rng.integers(0, 8, ndb), rng.integers(0, 3, ndb), rng.integers(0, 2, ndb), 3)
    pairs = np.stack([rng.integers(0, nq, 1500), rng.integers(0, ndb, 1500)], axis=1).astype(np.uint32)  # whole pairs repeat
    assert np.unique(pairs, axis=0).shape[0] < 1500
    got = check(ctx, pairs, q, db, span, max_gap, band)
    assert got.shape == (12,) and set(got["strand"].tolist()) == {0, 1}
    check(ctx, pairs, q, db, span, max_gap, band, min_seeds=3, upper=True)


def both_strands_equal():
    x, y, sb = [10, 30, 10, 30], [10, 30, 60, 40], [0, 0, 1, 1]
    return one_pair(x, y, sb)


def test_equal_best_scores_on_both_strands(ctx):
    assert check(ctx, *both_strands_equal(), 15, 100, 100).tolist() == [(0, 1, 0, 30, 2, 2, 10, 45, 10, 45)]
    assert check(ctx, *one_pair([0, 1], [0, 5]), 15, 100, 100).tolist() == [(0, 1, 0, 15, 1, 2, 0, 15, 0, 15)]
    assert check(ctx, *one_pair([0, 0, 20], [0, 1, 21]), 5, 100, 100).tolist() == [(0, 1, 0, 10, 2, 3, 0, 25, 1, 26)]
    assert check(ctx, *one_pair([0, 20, 500, 520], [0, 20, 500, 520]), 15, 50, 10).tolist() == [(0, 1, 0, 30, 2, 4, 0, 35, 0, 35)]


def random_batch(seed, n_pairs, n_reads=30, hi=2000):
    rng = np.random.default_rng(seed)
    n = 400
    q = side(rng.integers(0, hi, n), rng.integers(0, n_reads, n), rng.integers(0, 2, n), n_reads)
    db = side(rng.integers(0, hi, n), rng.integers(0, n_reads, n), rng.integers(0, 2, n), n_reads)
    return np.stack([rng.integers(0, n, n_pairs), rng.integers(0, n, n_pairs)], axis=1).astype(np.uint32), q, db


def test_order_independence(ctx):
    pairs, q, db = random_batch(5, 3000, n_reads=6, hi=300)
    first = check(ctx, pairs, q, db, 15, 60, 20)
    assert first["n_seeds"].max() > 2
    for seed in (1, 2, 3):
        again = ctx.seed_chains(np.ascontiguousarray(pairs[np.random.default_rng(seed).permutation(3000)]), q, db, 15, 60, 20)
        assert again.tobytes() == first.tobytes()


@pytest.mark.parametrize("n_pairs", [1023, 1024, 1025])
@pytest.mark.parametrize("upper", [False, True])
def test_entry_counts_across_a_sort_tile(ctx, n_pairs, upper):
    pairs, q, db = random_batch(n_pairs, n_pairs)
    check(ctx, pairs, q, db, 15, 500, 100, upper=upper)


@pytest.mark.parametrize("upper", [False, True])
def test_more_groups_than_one_grid_pass(ctx, upper):
    rng = np.random.default_rng(11)
    n_rp = 5000
    ra, rb = rng.integers(0, 3000, n_rp), rng.integers(0, 3000, n_rp)
    hits = rng.integers(1, 4, n_rp)
    groups = []
    for a, b, h in zip(ra.tolist(), rb.tolist(), hits.tolist()):
        for t in range(h):
            groups.append((a, b, int(rng.integers(0, 2)), [int(rng.integers(0, 60))], [int(rng.integers(0, 60))]))
    pairs, q, db = from_groups(groups, 3000)
    got = check(ctx, pairs[rng.permutation(pairs.shape[0])], q, db, 15, 40, 10, upper=upper)
    assert got.shape[0] > 2000 and (not upper or (got["read_a"] < got["read_b"]).all())


def test_filters_do_not_promote_a_runner_up(ctx):
    args = one_pair([10, 30, 50, 10, 30], [10, 30, 50, 60, 40], [0, 0, 0, 1, 1])
    assert check(ctx, *args, 15, 100, 100).tolist() == [(0, 1, 0, 45, 3, 3, 10, 65, 10, 65)]
    assert check(ctx, *args, 15, 100, 100, min_seeds=3, min_score=45).shape == (1,)
    assert check(ctx, *args, 15, 100, 100, min_seeds=4).shape == (0,)
    assert check(ctx, *args, 15, 100, 100, min_score=46).shape == (0,)
    pairs, q, db = random_batch(3, 2500, n_reads=8, hi=400)
    full = check(ctx, pairs, q, db, 15, 80, 30)
    some = check(ctx, pairs, q, db, 15, 80, 30, min_seeds=3, min_score=40)
    assert 0 < some.shape[0] < full.shape[0]


def test_alternating_with_anchor_overlaps_on_one_context():
    """kmu_anchor_overlaps and kmu_seed_chains group their entries in one workspace (kmu_runs.h): on a context of its own, a long
    call of one, a short and a long call of the other, a short call of the first.  No flag, keep word or start that a call left
    behind the next call's last entry may reach a record: each result equals its reference in every byte."""
    c = lib.Context(0)
    try:
        def overlaps(seed, n_pairs, strands):
            off, pairs, dist = random_case(np.random.default_rng(seed), n_pairs)
            want = reference_overlaps(pairs, dist, off, None, strands, 1, 1, False)
            got = c.anchor_overlaps(pairs, dist, off, strands=strands, band=1)
            assert want.shape[0] > 0 and got.tobytes() == want.tobytes()

        def chains(seed, n_pairs, upper):
            pairs, q, db = random_batch(seed, n_pairs)
            assert check(c, pairs, q, db, 15, 500, 100, upper=upper).shape[0] > 0

        overlaps(31, 513, 2)  # 1026 entries: just over a sort tile
        chains(32, 5, False)
        chains(33, 1025, True)
        overlaps(34, 3, 1)
    finally:
        c.close()


# ---- call forms -------------------------------------------------------------------------------------------------------------------
def raw(ctx, pairs, n_pairs, q, db, p, out, cap, mem=A.MEM_HOST, n_q=None, n_db=None):
    """the plain call: (status, n_out)"""
    ptr = lambda x: None if x is None else lib._ptr(x)[0]  # noqa: E731
    total = C.c_uint64(12345)
    rc = ctx.L.kmu_seed_chains(ctx.h, ptr(pairs), n_pairs, ptr(q.pos), ptr(q.read), ptr(q.strand),
                               q.pos.shape[0] if n_q is None else n_q, len(q.offsets) - 1, ptr(db.pos), ptr(db.read), ptr(db.strand),
                               db.pos.shape[0] if n_db is None else n_db, len(db.offsets) - 1,
                               None if p is None else C.byref(p), mem, ptr(out), cap, C.byref(total))
    return rc, int(total.value)


def params(**kw):
    d = dict(span=15, max_gap=500, band=100, min_seeds=1, min_score=0, max_pos=0, flags=0)
    d.update(kw)
    return A.ChainParams(*[d[n] for n, _ in A.ChainParams._fields_])


def test_count_only_cap_and_empty(ctx):
    pairs, q, db = random_batch(21, 900)
    want = reference_chains(pairs, q, db, 15, 500, 100)
    total = want.shape[0]
    assert total > 3
    assert raw(ctx, pairs, 900, q, db, params(), None, 0) == (A.OK, total)
    out = np.zeros(total, REC)
    assert raw(ctx, pairs, 900, q, db, params(), out, total - 1) == (A.E_BAD_ARG, total)
    assert raw(ctx, pairs, 900, q, db, params(), out, total) == (A.OK, total) and np.array_equal(out, want)
    out2 = np.zeros(total + 3, REC)
    assert raw(ctx, pairs, 900, q, db, params(), out2, total + 3) == (A.OK, total)
    assert np.array_equal(out2[:total], want) and out2[total:].tobytes() == bytes(3 * 40)
    assert raw(ctx, pairs, 0, q, db, params(), out, total) == (A.OK, 0)
    assert ctx.seed_chains(pairs[:0], q, db, 15, 500, 100).shape == (0,)
    # no strands: every anchor on strand 0
    qn, dbn = q._replace(strand=None), db._replace(strand=None)
    got = check(ctx, pairs, qn, dbn, 15, 500, 100)
    assert (got["strand"] == 0).all()
    check(ctx, pairs, q, dbn, 15, 500, 100)
    # a self-join on one set of arrays
    check(ctx, pairs, q, q, 15, 500, 100, upper=True)
    assert np.array_equal(ctx.seed_chains(pairs, q, None, 15, 500, 100), reference_chains(pairs, q, q, 15, 500, 100))


def test_device_tensors_give_the_same_records(ctx):
    import torch
    pairs, q, db = random_batch(22, 2000, n_reads=10, hi=500)
    dev = lambda x: torch.from_numpy(x.view({4: np.int32, 1: np.uint8, 8: np.int64}[x.dtype.itemsize])).cuda()  # noqa: E731
    dq, ddb = Side(dev(q.pos), dev(q.read), dev(q.strand), q.offsets), Side(dev(db.pos), dev(db.read), dev(db.strand), db.offsets)
    for kw in (dict(), dict(upper=True, min_seeds=2), dict(max_pos=499)):
        want = check(ctx, pairs, q, db, 15, 80, 30, **kw)
        got = ctx.seed_chains(dev(pairs), dq, ddb, 15, 80, 30, **kw)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (want.shape[0], 10)
        assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(lib.KmuError) as e:  # found on the device, refused at the call's synchronisation
        ctx.seed_chains(dev(pairs), dq, ddb, 15, 80, 30, max_pos=1)
    assert e.value.code == A.E_UNSUPPORTED


def test_max_pos_and_unsupported_input(ctx):
    pairs, q, db = random_batch(23, 1500, n_reads=10, hi=70000)
    top = int(max(q.pos[pairs[:, 0]].max(), db.pos[pairs[:, 1]].max()))
    plain = check(ctx, pairs, q, db, 21, 30000, 9000)
    for max_pos in (top, top + 1, 1 << 20, (1 << 31) - 1, (1 << 32) - 1):
        assert np.array_equal(check(ctx, pairs, q, db, 21, 30000, 9000, max_pos=max_pos), plain)
    uns = A.E_UNSUPPORTED
    assert raw(ctx, pairs, 1500, q, db, params(max_pos=top - 1), None, 0)[0] == uns
    worst = 7  # any pair: its entries get the positions at the edge of what the call takes
    far_q = q._replace(pos=q.pos.copy())
    far_q.pos[pairs[worst, 0]] = 1 << 31
    assert raw(ctx, pairs, 1500, far_q, db, params(), None, 0)[0] == uns
    far_q.pos[pairs[worst, 0]] = (1 << 31) - 1  # the largest position there is
    check(ctx, pairs, far_q, db, 21, 30000, 9000)
    far_db = db._replace(pos=db.pos.copy())
    far_db.pos[pairs[worst, 1]] = 1 << 31
    assert raw(ctx, pairs, 1500, q, far_db, params(), None, 0)[0] == uns
    far_db.pos[pairs[worst, 1]] = (1 << 31) - 1
    check(ctx, pairs, q, far_db, 21, 30000, 9000)
    check(ctx, pairs, far_q, far_db, 64, (1 << 32) - 1, (1 << 32) - 1)
    # entries and reads that do not exist are never used as an index
    assert raw(ctx, pairs, 1500, q, db, params(), None, 0, n_q=int(pairs[:, 0].max()))[0] == uns
    assert raw(ctx, pairs, 1500, q, db, params(), None, 0, n_db=int(pairs[:, 1].max()))[0] == uns
    few = q._replace(offsets=np.zeros(int(q.read[pairs[:, 0]].max()) + 1, np.uint64))
    assert raw(ctx, pairs, 1500, few, db, params(), None, 0)[0] == uns
    few = db._replace(offsets=np.zeros(int(db.read[pairs[:, 1]].max()) + 1, np.uint64))
    assert raw(ctx, pairs, 1500, q, few, params(), None, 0)[0] == uns
    assert np.array_equal(check(ctx, pairs, q, db, 21, 30000, 9000), plain)  # and the context still works


def test_argument_errors_launch_nothing(ctx):
    pairs, q, db = random_batch(24, 100)
    out = np.zeros(4, REC)
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        bad = A.E_BAD_ARG
        assert raw(ctx, None, 100, q, db, params(), out, 4)[0] == bad
        assert raw(ctx, pairs, 100, q._replace(pos=None), db, params(), out, 4, n_q=400)[0] == bad
        assert raw(ctx, pairs, 100, q._replace(read=None), db, params(), out, 4)[0] == bad
        assert raw(ctx, pairs, 100, q, db._replace(pos=None), params(), out, 4, n_db=400)[0] == bad
        assert raw(ctx, pairs, 100, q, db._replace(read=None), params(), out, 4)[0] == bad
        assert raw(ctx, pairs, 100, q, db, None, out, 4)[0] == bad
        for kw in (dict(span=0), dict(span=65), dict(max_gap=0), dict(min_seeds=0), dict(flags=2), dict(flags=A.CHAIN_UPPER | 0x100)):
            assert raw(ctx, pairs, 100, q, db, params(**kw), out, 4)[0] == bad, kw
        assert raw(ctx, pairs, 100, q, db, params(), out, 4, mem=7)[0] == bad
        assert raw(ctx, pairs, 100, q, db, params(), out, 4, n_q=0)[0] == bad
        assert raw(ctx, pairs, 100, q, db, params(), out, 4, n_db=0)[0] == bad
        assert raw(ctx, pairs, 100, q._replace(offsets=np.zeros(1, np.uint64)), db, params(), out, 4)[0] == bad
        assert raw(ctx, pairs, 100, q, db._replace(offsets=np.zeros(1, np.uint64)), params(), out, 4)[0] == bad
        assert raw(ctx, pairs, 1 << 32, q, db, params(), out, 4)[0] == A.E_UNSUPPORTED
        L = lib.load()
        assert L.kmu_seed_chains(ctx.h, lib._ptr(pairs)[0], 100, lib._ptr(q.pos)[0], lib._ptr(q.read)[0], None, 400, 30, lib._ptr(db.pos)[0],
                                 lib._ptr(db.read)[0], None, 400, 30, C.byref(params()), A.MEM_HOST, None, 0, None) == bad
        assert (out == np.zeros(4, REC)).all()
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        check(ctx, pairs, q, db, 15, 500, 100)
        prof = ctx.profile_get()
        for name in ("k_chain_keys_write", "k_chain_gather", "k_chain_heads", "k_chain_starts", "k_chain_dp", "k_chain_best_count",
                     "k_chain_best_write", "k_sort_scatter"):
            assert name in prof, name
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opposite", [False, True], ids=["same_strand", "opposite_strand"])
def test_two_reads_of_one_sequence(ctx, oracle, opposite):
    k, w, s, e = 15, 10, 1000, 2000
    genome = rand_reads(2024, [3000])[0]
    read_a, read_b = genome[0:e], genome[s:3000]  # they share genome[s:e): [s, e) of a, [0, e - s) of b
    len_b = len(read_b)
    reads = [read_a, revcomp(read_b) if opposite else read_b]
    bases, off = oracle.concat(reads)
    got = minimizer.read_chains(ctx, bases, off, k, w, fhash=A.FHASH_CANON_INVHASH)
    assert got.dtype == REC and got.shape == (1,)
    r = got[0]
    assert (r["read_a"], r["read_b"], r["strand"]) == (0, 1, int(opposite))
    b_start, b_end = (len_b - int(r["b_end"]), len_b - int(r["b_start"])) if opposite else (int(r["b_start"]), int(r["b_end"]))
    assert s <= r["a_start"] <= s + w - 1 and e - w + 1 <= r["a_end"] <= e
    assert 0 <= b_start <= w - 1 and e - s - w + 1 <= b_end <= e - s
    assert r["n_seeds"] >= (e - s - k - w + 1) / w
    # on the CPU: the oracle's hashes, the reference minimizers, a dict join and the reference chains give the same record, and
    # every anchor of the winning group lies on the true diagonal -- no chance hit joined the chain
    hashes, pos, read, strand, moff = expected(oracle, bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
    m = minimizer.Minimizers(hashes, pos, read, strand, moff, k, w, A.FHASH_CANON_INVHASH)
    hits = sorted(h for h in reference_hits(m, m, True, 0) if h[0] == 0)
    assert all((h[2] ^ h[5]) == int(opposite) and (h[1] + h[4] + k == len_b + s if opposite else h[1] - h[4] == s) for h in hits)
    assert len(hits) == r["n_anchors"] == r["n_seeds"]
    index = {(int(rd), int(p)): i for i, (rd, p) in enumerate(zip(read, pos))}
    pairs = np.array([(index[(h[0], h[1])], index[(h[3], h[4])]) for h in hits], np.uint32)
    want = reference_chains(pairs, m, m, k, 5000, 500, min_seeds=3, upper=True)
    assert np.array_equal(got, want)
    # the same on resident arrays
    import torch
    d = minimizer.read_chains(ctx, torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), k, w)
    assert d.is_cuda and d.cpu().numpy().tobytes() == got.tobytes()

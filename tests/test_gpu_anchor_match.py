"""-m gpu: kmu_anchor_match against a brute force over rows written here.

Expected result of a call: for every query row a and database row b whose key sets (the first min(n_keys, n) hashes) intersect and
whose groups differ, h* = min of the intersection (set arithmetic) and the triple oracle.minhash_distance(row_a[:n_a], row_b[:n_b]);
kept when common >= min_common; sorted by (a, h*, b).  The database keys sit in a dict so that the larger cases stay fast.  Pairs
and triples are compared exactly, the triples of the reported pairs also against ctx.minhash_distance_pairs, and every case
asserts that its expected list is not empty.  Rows are built directly in numpy, so the tests control the buckets.

Sizes: T = ANCHOR_SORT_TILE entries are ranked by one workgroup per radix pass, 64 candidates of a bucket are walked at a time,
and the two device scans (radix offsets over 256 x tiles counters, pair offsets over nq counts) change kernels above 32768 values."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib

pytestmark = pytest.mark.gpu
MAXH = np.uint64(0xFFFFFFFFFFFFFFFF)
T = A.ANCHOR_SORT_TILE


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def mk_rows(lists, m):
    """ascending hash lists -> rows padded with u64::MAX"""
    out = np.full((len(lists), m), MAXH, np.uint64)
    for r, hs in enumerate(lists):
        hs = sorted(int(h) for h in hs)
        assert len(set(hs)) == len(hs) <= m
        out[r, :len(hs)] = np.array(hs, np.uint64)
    return out


def pool_rows(rng, n_rows, m, pool, lens=None):
    """rows whose hashes are drawn from `pool` (sorted distinct u64 over the whole 64-bit range); lens: the n of every row"""
    if lens is None:
        lens = rng.integers(0, m + 1, n_rows)
    return mk_rows([rng.choice(pool, size=int(n), replace=False) for n in lens], m)


def make_pool(rng, size):
    p = np.unique(rng.integers(0, 0xFFFFFFFFFFFFFFFE, size=size, dtype=np.uint64, endpoint=True))
    return p


def brute(oracle, hq, hdb, n_keys, min_common, gq=None, gdb=None):
    nq_, ndb_ = (hq != MAXH).sum(axis=1), (hdb != MAXH).sum(axis=1)
    index = {}
    for b in range(hdb.shape[0]):
        for h in hdb[b, :min(n_keys, int(ndb_[b]))].tolist():
            index.setdefault(h, []).append(b)
    found = []
    for a in range(hq.shape[0]):
        keys_a = set(hq[a, :min(n_keys, int(nq_[a]))].tolist())
        cands = {b for h in keys_a for b in index.get(h, ())}
        for b in cands:
            if gq is not None and int(gq[a]) == int(gdb[b]):
                continue
            hstar = min(keys_a & set(hdb[b, :min(n_keys, int(ndb_[b]))].tolist()))
            d = oracle.minhash_distance(hq[a, :nq_[a]], hdb[b, :ndb_[b]])
            if d[0] >= min_common:
                found.append((a, hstar, b, d))
    found.sort(key=lambda x: x[:3])
    pairs = np.array([(a, b) for a, _, b, _ in found], np.uint32).reshape(-1, 2)
    dist = np.array([d for _, _, _, d in found], np.uint32).reshape(-1, 3)
    return pairs, dist


def check(ctx, oracle, hq, hdb, n_keys, min_common, gq=None, gdb=None):
    want_p, want_d = brute(oracle, hq, hdb, n_keys, min_common, gq, gdb)
    assert want_p.shape[0] > 0, "the case expects no pair: it would show nothing"
    got_p, got_d = ctx.anchor_match(hq, hdb, n_keys=n_keys, min_common=min_common, group_q=gq, group_db=gdb)
    assert got_p.dtype == np.uint32 and got_d.dtype == np.uint32
    assert got_p.shape == want_p.shape and np.array_equal(got_p, want_p)
    assert np.array_equal(got_d, want_d)
    again = ctx.minhash_distance_pairs(hq, hdb, np.ascontiguousarray(got_p[:, 0]), np.ascontiguousarray(got_p[:, 1]))
    assert np.array_equal(got_d, again)
    return got_p, got_d


# ---- buckets: the 64-candidate chunk and ordered compaction across chunks ---------------------------------------------------
def bucket_case(rng, sizes, m=16):
    """one query per bucket; the database rows of a bucket share the query's key and, at random, up to two more of its hashes,
    so that groups and min_common leave holes in every chunk"""
    q, db = [], []
    for i, size in enumerate(sizes):
        key = 1000 + i
        extra = [int(x) for x in rng.integers(1 << 20, 1 << 62, m - 1)]
        q.append([key] + extra)
        for _ in range(size):
            own = [int(x) for x in rng.integers(1 << 20, 1 << 62, m - 3)]
            db.append([key] + [e for e in extra[:2] if rng.random() < 0.5] + own)
    q.append([999] + [int(x) for x in rng.integers(1 << 20, 1 << 62, 3)])  # a key nobody has
    order = rng.permutation(len(db))  # buckets interleaved in row order: the sort has to gather them
    return mk_rows(q, m), mk_rows([db[i] for i in order], m)


@pytest.mark.parametrize("min_common", [0, 1, 3])
def test_buckets_across_the_chunk_boundary(ctx, oracle, min_common):
    rng = np.random.default_rng(11)
    hq, hdb = bucket_case(rng, [1, 2, 63, 64, 65, 130])
    got_p, _ = check(ctx, oracle, hq, hdb, 1, min_common)
    if min_common <= 1:
        assert np.bincount(got_p[:, 0], minlength=7).tolist() == [1, 2, 63, 64, 65, 130, 0]
    gq = np.arange(hq.shape[0], dtype=np.uint32) % 3
    gdb = (np.arange(hdb.shape[0], dtype=np.uint32) // 2) % 3
    check(ctx, oracle, hq, hdb, 1, min_common, gq, gdb)


# ---- the index at the sizes where the sort changes shape --------------------------------------------------------------------
# n_keys = 1: ndb * n_keys is T - 1, T, T + 1, 2T + 1.  n_keys = 4: T is a multiple of 4, so T - 1, T + 1 and 2T + 1 are not
# numbers of entries; the nearest ones on either side are taken (T - 4, T, T + 4, 2T + 4).
@pytest.mark.parametrize("n_keys,ndb", [(1, T - 1), (1, T), (1, T + 1), (1, 2 * T + 1),
                                        (4, T // 4 - 1), (4, T // 4), (4, T // 4 + 1), (4, T // 2 + 1)])
def test_index_sizes_around_the_sort_tile(ctx, oracle, n_keys, ndb):
    rng = np.random.default_rng(100 * n_keys + ndb)
    pool = make_pool(rng, 4 * ndb)
    m = 4
    # every database row is full, so the index holds ndb * n_keys real entries; short rows are test_row_shapes' business
    hdb = pool_rows(rng, ndb, m, pool, lens=np.full(ndb, m))
    hq = pool_rows(rng, 300, m, pool)
    check(ctx, oracle, hq, hdb, n_keys, 1)
    check(ctx, oracle, hq, hdb, n_keys, 0)


def test_every_radix_pass_matters(ctx, oracle):
    """keys that differ only in their top byte, only in their bottom byte, in one middle byte each, and keys 0 and 2^64 - 2"""
    keys = [0, 0xFFFFFFFFFFFFFFFE]
    keys += [b << 56 for b in (1, 2, 128, 255)]          # top byte only
    keys += [b for b in (1, 2, 128, 255)]                # bottom byte only
    keys += [0x0101010101010101 ^ (0xFF << (8 * p)) for p in range(8)]  # one byte apart from each other, in every position
    keys += [0xFFFFFFFFFFFFFF00 | b for b in (0, 1, 0xFD)]
    rng = np.random.default_rng(5)
    rows = [[k] for k in keys for _ in range(2)]  # two rows per key: the order by b inside a bucket
    hdb = mk_rows([rows[i] for i in rng.permutation(len(rows))], 2)
    hq = mk_rows([[k] for k in reversed(keys)], 2)
    got_p, got_d = check(ctx, oracle, hq, hdb, 1, 1)
    assert got_p.shape[0] == 2 * len(keys) and (got_d == 1).all()
    # two keys per query row: each meets the database rows of both, the smaller key's first
    ks = sorted(keys)
    hq2 = mk_rows([[ks[i], ks[i + 1]] for i in range(len(ks) - 1)], 2)
    got_p, _ = check(ctx, oracle, hq2, hdb, 2, 0)
    assert got_p.shape[0] == 4 * (len(ks) - 1)


# ---- row shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n_keys", [(1, 1), (16, 1), (16, 4), (16, 16), (256, 4), (256, 256)])
def test_row_shapes(ctx, oracle, m, n_keys):
    """n = 0, n < n_keys, n = m, and everything between; m of 1, 16 and 256"""
    rng = np.random.default_rng(1000 * m + n_keys)
    ndb, nq = 150, 90
    pool = make_pool(rng, max(3 * m, 400) if n_keys < 16 else 40 * m)
    lens = rng.integers(0, m + 1, ndb)
    lens[:6] = [0, m, min(1, m), max(n_keys - 1, 0), m, 0]
    hdb = pool_rows(rng, ndb, m, pool, lens=lens)
    lq = rng.integers(0, m + 1, nq)
    lq[:5] = [0, m, min(1, m), max(n_keys - 1, 0), min(2, m)]
    hq = pool_rows(rng, nq, m, pool, lens=lq)
    got_p, _ = check(ctx, oracle, hq, hdb, n_keys, 1)
    assert 0 not in got_p[:, 0].tolist() and not (set(got_p[:, 1].tolist()) & {0, 5})  # empty rows match nothing
    check(ctx, oracle, hq, hdb, n_keys, 0)


def test_a_pair_is_reported_once_under_its_smallest_shared_key(ctx, oracle):
    hq = mk_rows([[5, 7, 9, 11], [1, 7, 20, 40], [2, 5, 7, 50], [6, 8]], 4)
    hdb = mk_rows([[5, 7, 9, 12], [3, 7, 30, 41], [5, 6, 7, 60], [7, 100, 200, 300]], 4)
    got_p, got_d = check(ctx, oracle, hq, hdb, 4, 0)
    # (a, b) in the order (a, h*, b): row 0 meets 0 and 2 under 5, then 1 and 3 under 7; row 3 meets 2 under 6
    assert got_p.tolist() == [[0, 0], [0, 2], [0, 1], [0, 3], [1, 0], [1, 1], [1, 2], [1, 3],
                              [2, 0], [2, 2], [2, 1], [2, 3], [3, 2]]
    assert got_d[0].tolist() == [3, 4, 4]
    # with two keys per row, 7 is a key of rows 0 and 1 of both sides only where it is among the first two hashes
    check(ctx, oracle, hq, hdb, 2, 0)
    check(ctx, oracle, hq, hdb, 1, 0)


def test_a_candidate_whose_walk_finds_nothing(ctx, oracle):
    """n(a) = 2 against a full row: they share the key 10, the walk stops after two steps on the database row's smaller hashes"""
    hq = mk_rows([[10, 50], [1, 2, 3, 4, 5, 6, 7, 8]], 16)
    hdb = mk_rows([list(range(1, 17))], 16)
    got_p, got_d = check(ctx, oracle, hq, hdb, 16, 0)
    assert got_p.tolist() == [[0, 0], [1, 0]] and got_d[0].tolist() == [0, 2, 0]
    got_p, _ = check(ctx, oracle, hq, hdb, 16, 1)
    assert got_p.tolist() == [[1, 0]]


# ---- groups, self-join, two arrays, device tensors ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """rows of 40 'reads' of 5 slices each, over few enough hashes that many rows share several"""
    rng = np.random.default_rng(77)
    pool = make_pool(rng, 40)
    h = pool_rows(rng, 200, 8, pool, lens=rng.integers(0, 9, 200))
    return h, (np.arange(200, dtype=np.uint32) // 5)


@pytest.mark.parametrize("min_common", [0, 1, 3])
@pytest.mark.parametrize("n_keys", [1, 4])
def test_self_join_with_and_without_groups(ctx, oracle, batch, n_keys, min_common):
    h, group = batch
    got_p, got_d = check(ctx, oracle, h, h, n_keys, min_common, group, group)
    assert (group[got_p[:, 0]] != group[got_p[:, 1]]).all()
    fwd = {(a, b) for a, b in got_p.tolist()}
    if min_common == 0:  # both directions: sharing a key is symmetric (the walk's early stop is not: common may differ)
        assert fwd == {(b, a) for a, b in fwd}
    plain_p, _ = check(ctx, oracle, h, h, n_keys, min_common)
    assert plain_p.shape[0] > got_p.shape[0]  # every non-empty row meets itself, slices of one read meet each other


def test_two_different_arrays(ctx, oracle, batch):
    h, group = batch
    hq = np.ascontiguousarray(h[130:])
    hdb = np.ascontiguousarray(h[:150])
    check(ctx, oracle, hq, hdb, 4, 1, np.ascontiguousarray(group[130:]), np.ascontiguousarray(group[:150]))
    check(ctx, oracle, hq, hdb, 2, 0)


def test_device_tensors_give_the_same_arrays(ctx, oracle, batch):
    import torch
    h, group = batch
    want_p, want_d = ctx.anchor_match(h, h, n_keys=4, min_common=1, group_q=group, group_db=group)
    assert want_p.shape[0] > 0
    dh = torch.from_numpy(h.view(np.int64)).cuda()
    dg = torch.from_numpy(group.view(np.int32)).cuda()
    got_p, got_d = ctx.anchor_match(dh, dh, n_keys=4, min_common=1, group_q=dg, group_db=dg)
    assert got_p.is_cuda and got_d.is_cuda
    assert np.array_equal(got_p.cpu().numpy().view(np.uint32), want_p)
    assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d)
    dq = torch.from_numpy(np.ascontiguousarray(h[100:]).view(np.int64)).cuda()
    got_p, got_d = ctx.anchor_match(dq, dh, n_keys=1, min_common=0)
    want_p, want_d = brute(oracle, np.ascontiguousarray(h[100:]), h, 1, 0)
    assert want_p.shape[0] > 0
    assert np.array_equal(got_p.cpu().numpy().view(np.uint32), want_p) and np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d)


def test_both_scans_above_their_single_block_size(ctx, oracle):
    """ndb * n_keys = 160 000 entries are 157 tiles: 40 192 radix counters; 33 000 query rows: both above 32 768"""
    rng = np.random.default_rng(9)
    pool = make_pool(rng, 2_000_000)
    m = 4
    hdb = np.sort(pool[rng.integers(0, pool.size, (40_000, m))], axis=1)
    hdb = hdb[(np.diff(hdb, axis=1) != 0).all(axis=1)]  # (rows that drew a hash twice are dropped: distinct hashes)
    hq = np.sort(pool[rng.integers(0, pool.size, (33_000, m))], axis=1)
    hq = hq[(np.diff(hq, axis=1) != 0).all(axis=1)]
    assert hdb.shape[0] * 4 > 156 * T + 1 and hq.shape[0] > 32768
    got_p, _ = check(ctx, oracle, np.ascontiguousarray(hq), np.ascontiguousarray(hdb), 4, 1)
    assert got_p.shape[0] > 1000


# ---- sizes, the count-only call, argument errors ------------------------------------------------------------------------------
def raw(ctx, hq, nq, hdb, ndb, m, n_keys, min_common, gq, gdb, pairs, dist, cap, h=None):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_uint64(12345)
    rc = ctx.L.kmu_anchor_match(ctx.h if h is None else h, p(hq), nq, p(hdb), ndb, m, n_keys, min_common, p(gq), p(gdb), A.MEM_HOST,
                                p(pairs), p(dist), cap, C.byref(n))
    return rc, int(n.value)


def test_count_only_call_and_capacity(ctx, oracle, batch):
    h, group = batch
    want_p, want_d = brute(oracle, h, h, 4, 1, group, group)
    total = want_p.shape[0]
    assert total > 2
    assert raw(ctx, h, 200, h, 200, 8, 4, 1, group, group, None, None, 0) == (A.OK, total)
    pairs, dist = np.zeros((total, 2), np.uint32), np.zeros((total, 3), np.uint32)
    assert raw(ctx, h, 200, h, 200, 8, 4, 1, group, group, pairs, dist, total - 1) == (A.E_BAD_ARG, total)
    assert raw(ctx, h, 200, h, 200, 8, 4, 1, group, group, pairs, dist, total) == (A.OK, total)
    assert np.array_equal(pairs, want_p) and np.array_equal(dist, want_d)
    pairs2 = np.zeros((total + 5, 2), np.uint32)  # more room than needed, no triples wanted
    assert raw(ctx, h, 200, h, 200, 8, 4, 1, group, group, pairs2, None, total + 5) == (A.OK, total)
    assert np.array_equal(pairs2[:total], want_p) and (pairs2[total:] == 0).all()


def test_empty_sides_and_argument_errors(ctx, batch):
    h, group = batch
    m = h.shape[1]
    out = np.zeros((4, 2), np.uint32)
    assert raw(ctx, h, 0, h, 200, m, 1, 1, None, None, out, None, 4) == (A.OK, 0)
    assert raw(ctx, h, 200, h, 0, m, 1, 1, None, None, out, None, 4) == (A.OK, 0)
    p, d = ctx.anchor_match(h[:0], h)
    assert p.shape == (0, 2) and d.shape == (0, 3)
    p, d = ctx.anchor_match(h, h[:0])
    assert p.shape == (0, 2) and d.shape == (0, 3)
    assert (out == 0).all()
    bad = A.E_BAD_ARG
    assert raw(ctx, None, 200, h, 200, m, 1, 1, None, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, None, 200, m, 1, 1, None, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, h, 200, 0, 1, 1, None, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, h, 200, m, 0, 1, None, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, h, 200, m, m + 1, 1, None, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, h, 200, m, 1, 1, group, None, None, None, 0)[0] == bad
    assert raw(ctx, h, 200, h, 200, m, 1, 1, None, group, None, None, 0)[0] == bad
    L = lib.load()
    n = C.c_uint64(0)
    hp = h.ctypes.data_as(C.c_void_p)
    assert L.kmu_anchor_match(None, hp, 200, hp, 200, m, 1, 1, None, None, A.MEM_HOST, None, None, 0, C.byref(n)) == bad
    assert L.kmu_anchor_match(ctx.h, hp, 200, hp, 200, m, 1, 1, None, None, A.MEM_HOST, None, None, 0, None) == bad
    # unsupported sizes are refused before any row is read: the arrays may be short
    uns = A.E_UNSUPPORTED
    assert raw(ctx, h, 1, h, 1, A.ANCHOR_MAX_NBKMER + 1, 1, 1, None, None, None, None, 0)[0] == uns
    assert raw(ctx, h, 1, h, 1 << 30, 8, 4, 1, None, None, None, None, 0)[0] == uns          # ndb * n_keys == 2^32
    assert raw(ctx, h, 1, h, 0xFFFFFFFF, 8, 2, 1, None, None, None, None, 0)[0] == uns
    with pytest.raises(lib.KmuError) as e:
        ctx.anchor_match(h, h, n_keys=m + 1)
    assert e.value.code == bad


# ---- the directory of the database, built in the workspace for the one call ----------------------------------------------------
@pytest.mark.parametrize("n_keys", [1, 4])
@pytest.mark.parametrize("ndb", [1, 65])
def test_database_rows_all_empty(ctx, ndb, n_keys):
    """nothing but padding on the database side: a directory without a key, which only the device knows"""
    hq = mk_rows([[1, 2, 3, 4, 5], [7], list(range(10, 26))], 16)
    hdb = np.full((ndb, 16), MAXH, np.uint64)
    p, d = ctx.anchor_match(hq, hdb, n_keys=n_keys, min_common=0)
    assert p.shape == (0, 2) and d.shape == (0, 3)
    out = np.zeros((4, 2), np.uint32)
    assert raw(ctx, hq, 3, hdb, ndb, 16, n_keys, 0, None, None, out, None, 4) == (A.OK, 0)
    assert (out == 0).all()


def test_database_rows_shorter_than_n_keys_and_empty_rows(ctx, oracle):
    """short, empty and full database rows: their padding is sorted behind the real entries and is in no bucket"""
    rng = np.random.default_rng(55)
    pool = make_pool(rng, 600)
    lens = rng.integers(0, 17, 400)
    lens[:6] = [0, 3, 16, 0, 1, 2]
    lens[-1] = 0
    assert (lens < 4).sum() > 20 and (lens == 16).sum() > 5
    hdb = pool_rows(rng, 400, 16, pool, lens=lens)
    hq = pool_rows(rng, 80, 16, pool)
    got_p, _ = check(ctx, oracle, hq, hdb, 4, 1)
    assert not (set(got_p[:, 1].tolist()) & {0, 3, 399})  # empty rows match nothing
    check(ctx, oracle, hq, hdb, 4, 0)
    # a query row of nothing but padding asks for no key, and a full one's later hashes are not keys
    hq2 = np.concatenate([np.full((1, 16), MAXH, np.uint64), hq[:5]])
    got_p, _ = check(ctx, oracle, hq2, hdb, 4, 0)
    assert 0 not in got_p[:, 0].tolist()


def test_keys_the_directory_does_not_have(ctx, oracle):
    """query keys below the smallest database key, above the largest, and strictly between two neighbours, next to hits"""
    hdb = mk_rows([[100, 200, 900], [200, 300, 901], [300, 400, 902]], 4)  # keys (n_keys = 2): 100, 200, 300, 400
    hq = mk_rows([[5, 50, 200],       # both keys below the smallest
                  [500, 0xFFFFFFFFFFFFFFFE],  # both above the largest
                  [150, 250, 300],    # both between two neighbours (300 is its third hash: no key)
                  [99, 100, 200],     # a miss below, then a hit
                  [300, 350, 400],    # a hit, then a miss between
                  [400, 401],         # the largest key, then a miss above
                  [250, 300]], 4)     # a miss between, then a hit
    got_p, _ = check(ctx, oracle, hq, hdb, 2, 0)
    assert got_p.tolist() == [[3, 0], [4, 1], [4, 2], [5, 2], [6, 1], [6, 2]]
    check(ctx, oracle, hq, hdb, 1, 0)


def test_the_workspace_directory_and_an_index_do_not_meet(oracle):
    """an index owns its directory: a one-shot call that grows and overwrites the workspace in between leaves it alone (a context
    of its own, so that the workspace is as small as the index's build left it)"""
    rng = np.random.default_rng(31)
    pool = make_pool(rng, 500)
    ha = pool_rows(rng, 70, 8, pool, lens=rng.integers(1, 9, 70))
    pool_b = make_pool(rng, 9000)
    hb = pool_rows(rng, 3000, 8, pool_b, lens=np.full(3000, 8))
    hq = pool_rows(rng, 60, 8, np.concatenate([pool, pool_b[:200]]))
    want_p, want_d = brute(oracle, hq, ha, 4, 1)
    assert want_p.shape[0] > 0
    ctx = lib.Context(0)
    try:
        with ctx.anchor_index(ha, n_keys=4) as index:
            check(ctx, oracle, hq, hb, 4, 0)
            got_p, got_d = index.match(hq, min_common=1)
            assert np.array_equal(got_p, want_p) and np.array_equal(got_d, want_d)
            one_p, one_d = ctx.anchor_match(hq, ha, n_keys=4, min_common=1)
            assert np.array_equal(one_p, got_p) and np.array_equal(one_d, got_d)
    finally:
        ctx.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_read_anchors_then_match(ctx, oracle):
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    genome = bytes(rng.choice(acgt, size=3000))
    reads = [genome[:3000], genome[:1500]] + [bytes(rng.choice(acgt, size=int(n))) for n in (1200, 700, 90)]
    bases, off = oracle.concat(reads)
    params = anchor.AnchorsGeneratorParameters("reads.fasta", 500, 16, 21, 250)
    hashes, _, n, row_off = ctx.read_anchors(bases, off, params.sketch_params(), 500, 250, want_counts=False)
    group = np.repeat(np.arange(len(reads), dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    for n_keys, min_common in ((1, 1), (4, 1), (4, 0), (1, 3)):
        want_p, want_d = brute(oracle, hashes, hashes, n_keys, min_common, group, group)
        assert want_p.shape[0] > 0
        rec = anchor.match_read_anchors(ctx, hashes, row_off, params, n_keys=n_keys, min_common=min_common, first_readnum=10)
        wa = anchor.rows_to_slices(want_p[:, 0], row_off, 250, 10)
        wb = anchor.rows_to_slices(want_p[:, 1], row_off, 250, 10)
        want = np.stack([wa[0], wa[1], wb[0], wb[1], want_d[:, 0].astype(np.int64), want_d[:, 1].astype(np.int64)], axis=1)
        assert np.array_equal(rec, want)
        got = {tuple(r) for r in rec.tolist()}
        for pos in (0, 250, 500):  # the same 500 bases in both reads: identical rows
            assert (10, pos, 11, pos, 16, 16) in got and (11, pos, 10, pos, 16, 16) in got
    # the rows on the device: the same records
    import torch
    dh = torch.from_numpy(np.ascontiguousarray(hashes).view(np.int64)).cuda()
    assert np.array_equal(anchor.match_read_anchors(ctx, dh, row_off, params, n_keys=4, min_common=1, first_readnum=10),
                          anchor.match_read_anchors(ctx, hashes, row_off, params, n_keys=4, min_common=1, first_readnum=10))

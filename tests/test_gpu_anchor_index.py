"""-m gpu: the anchor index (kmu_anchor_index_*) against a brute force over rows written here.

Expected result of a match: occ(h) = the database rows that have h among their keys (the first min(n_keys, n) hashes); h is masked
iff max_occ > 0 and occ(h) > max_occ; for every query row a and database row b whose groups differ, U = the unmasked hashes of
keys(a) & keys(b); a pair iff U is not empty, under h* = min U, with the triple oracle.minhash_distance(row_a[:n_a], row_b[:n_b])
over the whole rows, kept when common >= min_common; sorted by (a, h*, b).  The database keys sit in a dict (as `brute` of
test_gpu_anchor_match.py has them) so that the larger cases stay fast.  Pairs and triples are compared exactly and every case that
expects pairs asserts that the brute force found some.  Rows are built directly in numpy, so the tests control the buckets.

Sizes: T = ANCHOR_SORT_TILE entries are ranked by one workgroup per radix pass, 64 candidates of a bucket are walked at a time and
64 keys of a row are looked up at a time, and the device scan behind the directory changes kernels above 32768 values."""
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


def make_pool(rng, size):
    return np.unique(rng.integers(0, 0xFFFFFFFFFFFFFFFE, size=size, dtype=np.uint64, endpoint=True))


def pool_rows(rng, n_rows, m, pool, lens=None):
    """rows whose hashes are drawn from `pool`; lens: the n of every row"""
    if lens is None:
        lens = rng.integers(0, m + 1, n_rows)
    return mk_rows([rng.choice(pool, size=int(n), replace=False) for n in lens], m)


def db_keys(hdb, n_keys):
    """{hash: [database rows that have it among their keys], ascending}"""
    n = (hdb != MAXH).sum(axis=1)
    index = {}
    for b in range(hdb.shape[0]):
        for h in hdb[b, :min(n_keys, int(n[b]))].tolist():
            index.setdefault(h, []).append(b)
    return index


def brute(oracle, hq, hdb, n_keys, min_common, gq=None, gdb=None, max_occ=0):
    nq_, ndb_ = (hq != MAXH).sum(axis=1), (hdb != MAXH).sum(axis=1)
    index = db_keys(hdb, n_keys)
    seeds = {h: rows for h, rows in index.items() if not (max_occ > 0 and len(rows) > max_occ)}  # occupancy: database rows only
    found = []
    for a in range(hq.shape[0]):
        keys_a = set(hq[a, :min(n_keys, int(nq_[a]))].tolist()) & seeds.keys()
        cands = {b for h in keys_a for b in seeds[h]}
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


def check(index, oracle, hq, hdb, n_keys, min_common, gq=None, gdb=None, max_occ=0, expect_pairs=True):
    want_p, want_d = brute(oracle, hq, hdb, n_keys, min_common, gq, gdb, max_occ)
    if expect_pairs:
        assert want_p.shape[0] > 0, "the case expects no pair: it would show nothing"
    got_p, got_d = index.match(hq, group_q=gq, min_common=min_common, max_occ=max_occ)
    assert got_p.dtype == np.uint32 and got_d.dtype == np.uint32
    assert got_p.shape == want_p.shape and np.array_equal(got_p, want_p)
    assert got_d.shape == want_d.shape and np.array_equal(got_d, want_d)
    return got_p, got_d


SIZES = [1, 2, 63, 64, 65, 130]


def bucket_case(rng, sizes, m=16):
    """one query per bucket; the database rows of a bucket share the query's key and, at random, up to two more of its hashes,
    so that groups and min_common leave holes in every chunk; the buckets are interleaved in row order"""
    q, db = [], []
    for i, size in enumerate(sizes):
        key = 1000 + i
        extra = [int(x) for x in rng.integers(1 << 20, 1 << 62, m - 1)]
        q.append([key] + extra)
        for _ in range(size):
            own = [int(x) for x in rng.integers(1 << 20, 1 << 62, m - 3)]
            db.append([key] + [e for e in extra[:2] if rng.random() < 0.5] + own)
    q.append([999] + [int(x) for x in rng.integers(1 << 20, 1 << 62, 3)])  # a key nobody has
    order = rng.permutation(len(db))
    return mk_rows(q, m), mk_rows([db[i] for i in order], m)


@pytest.fixture(scope="module")
def buckets():
    hq, hdb = bucket_case(np.random.default_rng(11), SIZES)
    gq = np.arange(hq.shape[0], dtype=np.uint32) % 3
    gdb = (np.arange(hdb.shape[0], dtype=np.uint32) // 2) % 3
    return hq, hdb, gq, gdb


# ---- 1. max_occ = 0 is anchor_match ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_common", [0, 1, 3])
@pytest.mark.parametrize("groups", [False, True])
def test_without_a_mask_the_index_is_anchor_match(ctx, oracle, buckets, groups, min_common):
    hq, hdb, gq, gdb = buckets
    if not groups:
        gq = gdb = None
    with ctx.anchor_index(hdb, n_keys=1, group_db=gdb) as index:
        got_p, got_d = check(index, oracle, hq, hdb, 1, min_common, gq, gdb)
    ref_p, ref_d = ctx.anchor_match(hq, hdb, n_keys=1, min_common=min_common, group_q=gq, group_db=gdb)
    assert np.array_equal(got_p, ref_p) and np.array_equal(got_d, ref_d)
    if not groups and min_common <= 1:
        assert np.bincount(got_p[:, 0], minlength=7).tolist() == SIZES + [0]


# ---- 2. the mask boundary -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_occ", [1, 63, 64, 65, 130, 131])
def test_the_mask_boundary(ctx, oracle, buckets, max_occ):
    hq, hdb, gq, gdb = buckets
    with ctx.anchor_index(hdb, n_keys=1) as index:
        assert index.info()["max_occupancy"] == 130
        plain_p, plain_d = index.match(hq, min_common=0, max_occ=0)
        got_p, got_d = check(index, oracle, hq, hdb, 1, 0, max_occ=max_occ)
        keep = np.isin(plain_p[:, 0], [i for i, size in enumerate(SIZES) if size <= max_occ])
        assert np.array_equal(got_p, plain_p[keep]) and np.array_equal(got_d, plain_d[keep])
        assert np.bincount(got_p[:, 0], minlength=7).tolist() == [s if s <= max_occ else 0 for s in SIZES] + [0]
        if max_occ >= 130:
            assert np.array_equal(got_p, plain_p)
    with ctx.anchor_index(hdb, n_keys=1, group_db=gdb) as index:
        check(index, oracle, hq, hdb, 1, 1, gq, gdb, max_occ=max_occ, expect_pairs=max_occ > 1)  # (the bucket of one: same group)


# ---- 3. h* under a mask ---------------------------------------------------------------------------------------------------------
def test_the_smallest_unmasked_shared_key_names_the_pair(ctx, oracle):
    """10 and 30 are carried by more than two database rows (masked at max_occ = 2); 5, 7, 15, 20, 40 by one each"""
    u = iter(range(1000, 100000, 7))  # hashes nobody shares
    hq = mk_rows([[10, 15, 20, next(u)],          # a0
                  [10, next(u), next(u), next(u)],  # a1
                  [5, 30, next(u), next(u)],      # a2
                  [7, 10, 40, next(u)]], 4)       # a3
    db = [[10, 20, next(u), next(u)],             # b0: shares masked 10 and unmasked 20 with a0
          [10, next(u), next(u), next(u)],        # b1: shares only masked 10, with a0, a1 and a3
          [5, 30, next(u), next(u)],              # b2: unmasked 5 in front of masked 30, with a2
          [7, 10, 40, next(u)],                   # b3: unmasked 7 and 40 around masked 10, with a3
          [15, next(u), next(u), next(u)]]        # b4: unmasked 15 with a0, in front of 20 in the order
    db += [[10, next(u), next(u), next(u)] for _ in range(3)] + [[30, next(u), next(u), next(u)] for _ in range(3)]
    hdb = mk_rows(db, 4)
    with ctx.anchor_index(hdb, n_keys=4) as index:
        got_p, got_d = check(index, oracle, hq, hdb, 4, 0, max_occ=2)
        # a0: b4 under 15, then b0 under 20 (not under 10, where it stands without a mask); a1: nothing; a2: b2 under 5;
        # a3: b3 once, under 7
        assert got_p.tolist() == [[0, 4], [0, 0], [2, 2], [3, 3]]
        assert got_d.tolist() == [[1, 4, 4], [2, 4, 4], [2, 4, 4], [3, 4, 4]]  # the walks see the masked hashes too
        plain_p, _ = check(index, oracle, hq, hdb, 4, 0)
        assert plain_p[:3].tolist() == [[0, 0], [0, 1], [0, 3]] and plain_p.shape[0] > got_p.shape[0]
        assert plain_p.tolist().count([3, 3]) == 1
        check(index, oracle, hq, hdb, 4, 3, max_occ=2)  # min_common on top: (a3, b3) alone


# ---- 4. occupancy counts database rows only -------------------------------------------------------------------------------------
def test_query_rows_do_not_count_towards_the_occupancy(ctx, oracle):
    rng = np.random.default_rng(4)
    pool = make_pool(rng, 4000)
    key = int(pool[0])  # the smallest hash of the pool: the first key of every row that has it
    hq = mk_rows([[key] + rng.choice(pool[1:], 3, replace=False).tolist() for _ in range(100)], 4)
    hdb = mk_rows([[key] + rng.choice(pool[1:], 3, replace=False).tolist() for _ in range(2)]
                  + [rng.choice(pool[1:], 4, replace=False).tolist() for _ in range(30)], 4)
    with ctx.anchor_index(hdb, n_keys=1) as index:
        got_p, _ = check(index, oracle, hq, hdb, 1, 0, max_occ=2)
        assert got_p.shape[0] == 200
        got_p, _ = check(index, oracle, hq, hdb, 1, 0, max_occ=1, expect_pairs=False)
        assert got_p.shape[0] == 0


# ---- 5. directory shapes --------------------------------------------------------------------------------------------------------
def check_info(index, hdb, n_keys, groups=False):
    n = (hdb != MAXH).sum(axis=1)
    keys = np.concatenate([hdb[b, :min(n_keys, int(n[b]))] for b in range(hdb.shape[0])] + [np.zeros(0, np.uint64)])
    uniq, counts = np.unique(keys, return_counts=True)
    info = index.info()
    assert (info["ndb"], info["m"], info["n_keys"], info["has_groups"]) == (hdb.shape[0], hdb.shape[1], n_keys, int(groups))
    assert info["n_entries"] == keys.size == int(np.minimum(n, n_keys).sum())
    assert info["n_distinct"] == uniq.size
    assert info["max_occupancy"] == (int(counts.max()) if counts.size else 0)
    assert info["device_bytes"] >= hdb.size * 8
    return counts


@pytest.mark.parametrize("equal", [False, True])
@pytest.mark.parametrize("ndb", [T - 1, T, T + 1, 2 * T + 1])
def test_directory_sizes_around_the_sort_tile(ctx, oracle, ndb, equal):
    rng = np.random.default_rng(ndb)
    pool = make_pool(rng, 8 * ndb)
    hdb = np.sort(pool[rng.permutation(pool.size)[:4 * ndb]].reshape(ndb, 4), axis=1)  # every hash once: all first keys differ
    if equal:
        hdb[:, 0] = pool[0] if pool[0] < hdb.min() else np.uint64(0)
        assert (np.diff(hdb.astype(object), axis=1) > 0).all()
    hq = np.ascontiguousarray(hdb[rng.integers(0, ndb, 3)])
    with ctx.anchor_index(hdb, n_keys=1) as index:
        counts = check_info(index, hdb, 1)
        assert counts.tolist() == ([ndb] if equal else [1] * ndb)
        got_p, _ = check(index, oracle, hq, hdb, 1, 1)
        assert got_p.shape[0] == (3 * ndb if equal else 3)


def test_rows_shorter_than_n_keys_and_empty_rows(ctx, oracle):
    rng = np.random.default_rng(55)
    pool = make_pool(rng, 300)
    lens = rng.integers(0, 9, 400)
    lens[:4] = [0, 3, 8, 0]
    lens[-1] = 0
    hdb = pool_rows(rng, 400, 8, pool, lens=lens)
    hq = pool_rows(rng, 80, 8, pool)
    with ctx.anchor_index(hdb, n_keys=4) as index:
        check_info(index, hdb, 4)
        got_p, _ = check(index, oracle, hq, hdb, 4, 1)
        assert not (set(got_p[:, 1].tolist()) & {0, 3, 399})  # empty rows match nothing
        occ = max(len(v) for v in db_keys(hdb, 4).values())
        check(index, oracle, hq, hdb, 4, 0, max_occ=occ // 2)
    empty = np.full((5, 8), MAXH, np.uint64)
    with ctx.anchor_index(empty, n_keys=4) as index:  # nothing but padding: an index without a key
        assert check_info(index, empty, 4).size == 0
        assert index.occupancy(4).tolist() == [0, 0, 0, 0]
        assert index.match(hq)[0].shape == (0, 2)


def test_a_directory_above_the_single_block_of_the_scan(ctx, oracle):
    """40 000 rows, one key each: 40 000 flags, above the 32 768 values one block of the scan takes, and 34 000 distinct keys"""
    rng = np.random.default_rng(9)
    pool = make_pool(rng, 200_000)
    small, large = pool[:34_000], pool[34_000:]  # every first key is smaller than every other hash
    firsts = rng.permutation(np.concatenate([small, rng.choice(small[:2000], 6000)]))  # 6000 rows share their key with others
    rest = np.sort(large[rng.integers(0, large.size, (40_000, 3))], axis=1)
    hdb = np.concatenate([firsts[:, None], rest], axis=1)
    hdb = np.ascontiguousarray(hdb[(np.diff(rest, axis=1) != 0).all(axis=1)])  # (rows that drew a hash twice are dropped)
    assert hdb.shape[0] > 39_000
    hq = np.ascontiguousarray(hdb[rng.integers(0, hdb.shape[0], 300)])
    with ctx.anchor_index(hdb, n_keys=1) as index:
        counts = check_info(index, hdb, 1)
        assert counts.size > 32768 and counts.max() >= 3
        hist = index.occupancy(int(counts.max()) + 1)
        assert hist.tolist() == np.bincount(counts).tolist()
        check(index, oracle, hq, hdb, 1, 1)
        check(index, oracle, hq, hdb, 1, 1, max_occ=1)


# ---- 6. the occupancy histogram -------------------------------------------------------------------------------------------------
def test_occupancy_histogram(ctx, buckets):
    _, hdb, _, _ = buckets
    for n_keys in (1, 4):
        sizes = np.array([len(v) for v in db_keys(hdb, n_keys).values()])
        with ctx.anchor_index(hdb, n_keys=n_keys) as index:
            top = index.info()["max_occupancy"]
            assert top == sizes.max() == 130
            for n_bins in (2, 3, top + 1, top + 10):
                want = np.bincount(np.minimum(sizes, n_bins - 1), minlength=n_bins)
                hist = index.occupancy(n_bins)
                assert hist.dtype == np.uint64 and hist.tolist() == want.tolist() and hist[0] == 0
            assert anchor.max_occ_for_fraction(index.occupancy(top + 1), 0) == top


def test_occupancy_above_the_bins_kept_in_lds(ctx):
    """one key of 1500 rows next to 200 keys of one row: bins beyond the 1024 that a workgroup keeps"""
    hdb = mk_rows([[7, 100 + b] for b in range(1500)] + [[10_000 + b, 20_000 + b] for b in range(200)], 2)
    with ctx.anchor_index(hdb, n_keys=1) as index:
        assert index.info()["max_occupancy"] == 1500
        hist = index.occupancy(1501)
        assert hist[1] == 200 and hist[1500] == 1 and hist.sum() == 201
        assert index.occupancy(1200).tolist() == [0, 200] + [0] * 1197 + [1]
        assert index.occupancy(2).tolist() == [0, 201]


# ---- 7. the index is resident and its own ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch():
    """rows of 40 'reads' of 5 slices each, over few enough hashes that many rows share several"""
    rng = np.random.default_rng(77)
    pool = make_pool(rng, 40)
    h = pool_rows(rng, 200, 8, pool, lens=rng.integers(0, 9, 200))
    return h, (np.arange(200, dtype=np.uint32) // 5)


def test_the_index_is_resident_and_its_own(ctx, oracle, batch):
    h, group = batch
    rng = np.random.default_rng(3)
    hdb, gdb = np.ascontiguousarray(h[:150]), np.ascontiguousarray(group[:150])
    mine, mine_g = hdb.copy(), gdb.copy()
    index = ctx.anchor_index(mine, n_keys=4, group_db=mine_g)
    mine[:] = 12345  # the caller's arrays are the caller's again
    mine_g[:] = 7
    other = ctx.anchor_index(np.ascontiguousarray(h[100:]), n_keys=2)  # two indexes alive at once
    queries = [(np.ascontiguousarray(h[130:]), np.ascontiguousarray(group[130:])),
               (np.ascontiguousarray(h[:60]), np.ascontiguousarray(group[:60])),
               (np.ascontiguousarray(h[50:170]), np.ascontiguousarray(group[50:170]))]
    for i, (hq, gq) in enumerate(queries):
        got = check(index, oracle, hq, hdb, 4, 1, gq, gdb, max_occ=(0, 6, 3)[i])
        with ctx.anchor_index(hdb, n_keys=4, group_db=gdb) as fresh:
            again = fresh.match(hq, group_q=gq, min_common=1, max_occ=(0, 6, 3)[i])
        assert np.array_equal(got[0], again[0]) and np.array_equal(got[1], again[1])
        check(other, oracle, hq, np.ascontiguousarray(h[100:]), 2, 0)
        # other calls that use the shared workspace, between two matches
        big = pool_rows(rng, 600, 8, make_pool(rng, 200))
        assert ctx.anchor_match(big, big, n_keys=4, min_common=0)[0].shape[0] > 600
        bases, off = oracle.concat([bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=2000))])
        params = anchor.AnchorsGeneratorParameters("x", 500, 16, 21, 250)
        assert ctx.read_anchors(bases, off, params.sketch_params(), 500, 250, want_counts=False)[0].shape == (8, 16)
    other.close()
    index.close()
    index.close()  # closing twice is harmless


# ---- 8. device tensors, the count-only call, sizes, argument errors ---------------------------------------------------------------
def test_device_tensors_give_the_same_arrays(ctx, oracle, batch):
    import torch
    h, group = batch
    dh = torch.from_numpy(h.view(np.int64)).cuda()
    dg = torch.from_numpy(group.view(np.int32)).cuda()
    with ctx.anchor_index(h, n_keys=4, group_db=group) as host_index, ctx.anchor_index(dh, n_keys=4, group_db=dg) as dev_index:
        assert host_index.info() == dev_index.info()
        assert dev_index.occupancy(9).tolist() == host_index.occupancy(9).tolist()
        for max_occ in (0, 5):
            want_p, want_d = check(host_index, oracle, h, h, 4, 1, group, group, max_occ=max_occ)
            for index in (host_index, dev_index):  # the query's side is free of the side the index was built from
                got_p, got_d = index.match(dh, group_q=dg, min_common=1, max_occ=max_occ)
                assert got_p.is_cuda and got_d.is_cuda
                assert np.array_equal(got_p.cpu().numpy().view(np.uint32), want_p)
                assert np.array_equal(got_d.cpu().numpy().view(np.uint32), want_d)
            got_p, got_d = dev_index.match(h, group_q=group, min_common=1, max_occ=max_occ)
            assert np.array_equal(got_p, want_p) and np.array_equal(got_d, want_d)
        hist = torch.zeros(9, dtype=torch.int64, device="cuda")
        assert ctx.L.kmu_anchor_index_occupancy(dev_index.h, C.c_void_p(hist.data_ptr()), 9, A.MEM_DEVICE) == A.OK
        ctx.synchronize()
        assert hist.cpu().numpy().tolist() == host_index.occupancy(9).tolist()


def raw_match(ctx, index, hq, nq, gq, min_common, max_occ, pairs, dist, cap, mem=A.MEM_HOST, n_out=True):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = C.c_uint64(12345)
    rc = ctx.L.kmu_anchor_index_match(index, p(hq), nq, p(gq), min_common, max_occ, mem, p(pairs), p(dist), cap,
                                      C.byref(n) if n_out else None)
    return rc, int(n.value)


def test_count_only_call_and_capacity(ctx, oracle, batch):
    h, group = batch
    want_p, want_d = brute(oracle, h, h, 4, 1, group, group, max_occ=5)
    total = want_p.shape[0]
    assert total > 2
    with ctx.anchor_index(h, n_keys=4, group_db=group) as index:
        assert raw_match(ctx, index.h, h, 200, group, 1, 5, None, None, 0) == (A.OK, total)
        pairs, dist = np.zeros((total, 2), np.uint32), np.zeros((total, 3), np.uint32)
        assert raw_match(ctx, index.h, h, 200, group, 1, 5, pairs, dist, total - 1) == (A.E_BAD_ARG, total)
        assert raw_match(ctx, index.h, h, 200, group, 1, 5, pairs, dist, total) == (A.OK, total)
        assert np.array_equal(pairs, want_p) and np.array_equal(dist, want_d)
        pairs2 = np.zeros((total + 5, 2), np.uint32)  # more room than needed, no triples wanted
        assert raw_match(ctx, index.h, h, 200, group, 1, 5, pairs2, None, total + 5) == (A.OK, total)
        assert np.array_equal(pairs2[:total], want_p) and (pairs2[total:] == 0).all()


def raw_create(ctx, hdb, ndb, m, n_keys, gdb, mem=A.MEM_HOST, h="ctx", out=True):
    p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    ix = C.c_void_p()
    rc = ctx.L.kmu_anchor_index_create(ctx.h if h == "ctx" else h, p(hdb), ndb, m, n_keys, p(gdb), mem, C.byref(ix) if out else None)
    return rc, ix


def test_empty_sides_and_argument_errors(ctx, batch):
    h, group = batch
    m = h.shape[1]
    out = np.zeros((4, 2), np.uint32)
    with ctx.anchor_index(h[:0], n_keys=2) as index:  # ndb = 0: a valid index that matches nothing
        info = index.info()
        assert (info["ndb"], info["n_entries"], info["n_distinct"], info["max_occupancy"]) == (0, 0, 0, 0)
        assert index.occupancy(3).tolist() == [0, 0, 0]
        p, d = index.match(h, max_occ=3)
        assert p.shape == (0, 2) and d.shape == (0, 3)
        assert raw_match(ctx, index.h, h, 200, None, 1, 0, out, None, 4) == (A.OK, 0)
    bad, uns = A.E_BAD_ARG, A.E_UNSUPPORTED
    with ctx.anchor_index(h, n_keys=2) as plain, ctx.anchor_index(h, n_keys=2, group_db=group) as grouped:
        p, d = plain.match(h[:0])  # nq = 0
        assert p.shape == (0, 2) and d.shape == (0, 3)
        assert raw_match(ctx, plain.h, h, 0, None, 1, 0, out, None, 4) == (A.OK, 0)
        assert (out == 0).all()
        # match: nulls, bad mem, groups on one side only
        assert raw_match(ctx, None, h, 200, None, 1, 0, None, None, 0)[0] == bad
        assert raw_match(ctx, plain.h, None, 200, None, 1, 0, None, None, 0)[0] == bad
        assert raw_match(ctx, plain.h, h, 200, None, 1, 0, None, None, 0, n_out=False)[0] == bad
        assert raw_match(ctx, plain.h, h, 200, None, 1, 0, None, None, 0, mem=7)[0] == bad
        assert raw_match(ctx, plain.h, h, 200, group, 1, 0, None, None, 0)[0] == bad
        assert raw_match(ctx, grouped.h, h, 200, None, 1, 0, None, None, 0)[0] == bad
        with pytest.raises(lib.KmuError) as e:
            plain.match(h, group_q=group)
        assert e.value.code == bad
        with pytest.raises(ValueError):
            plain.match(np.ascontiguousarray(h[:, :4]))
        # occupancy and info
        hist = np.zeros(8, np.uint64)
        hp = hist.ctypes.data_as(C.c_void_p)
        assert ctx.L.kmu_anchor_index_occupancy(None, hp, 8, A.MEM_HOST) == bad
        assert ctx.L.kmu_anchor_index_occupancy(plain.h, None, 8, A.MEM_HOST) == bad
        assert ctx.L.kmu_anchor_index_occupancy(plain.h, hp, 1, A.MEM_HOST) == bad
        assert ctx.L.kmu_anchor_index_occupancy(plain.h, hp, 65537, A.MEM_HOST) == bad
        assert ctx.L.kmu_anchor_index_occupancy(plain.h, hp, 8, 7) == bad
        assert ctx.L.kmu_anchor_index_info(None, C.byref(A.AnchorIndexInfo())) == bad
        assert ctx.L.kmu_anchor_index_info(plain.h, None) == bad
    # create
    assert raw_create(ctx, h, 200, m, 1, None, h=None)[0] == bad
    assert raw_create(ctx, None, 200, m, 1, None)[0] == bad
    assert raw_create(ctx, h, 200, m, 1, None, out=False)[0] == bad
    assert raw_create(ctx, h, 200, 0, 1, None)[0] == bad
    assert raw_create(ctx, h, 200, m, 0, None)[0] == bad
    assert raw_create(ctx, h, 200, m, m + 1, None)[0] == bad
    assert raw_create(ctx, h, 200, m, 1, None, mem=7)[0] == bad
    # unsupported sizes are refused before any row is read: the arrays may be short
    assert raw_create(ctx, h, 1, A.ANCHOR_MAX_NBKMER + 1, 1, None)[0] == uns
    assert raw_create(ctx, h, 1 << 30, 8, 4, None)[0] == uns  # ndb * n_keys == 2^32
    rc, ix = raw_create(ctx, h, 0xFFFFFFFF, 8, 2, None)
    assert rc == uns and not ix.value
    ctx.L.kmu_anchor_index_destroy(None)  # a no-op
    with pytest.raises(lib.KmuError) as e:
        ctx.anchor_index(h, n_keys=m + 1)
    assert e.value.code == bad


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------
WINDOW, OVERLAP, NBKMER, K = 500, 250, 16, 21
STRIDE = WINDOW - OVERLAP


def polya_reads():
    """Seven reads of 1500 bases tiled every 250 bases over a random genome of 3000, a stretch of 600 A inserted into every one
    at its base 1000: the three whole windows in front of the insert are plain genome, and two reads whose starts lie 250 bases
    apart share two of them."""
    rng = np.random.default_rng(2026)
    genome = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000))
    reads = []
    for start in range(0, 1501, 250):
        r = genome[start:start + 1500]
        reads.append(r[:1000] + b"A" * 600 + r[1000:])
    return reads


def windows_of(read):
    """the bases of every slice, by the rule of kmu_read_anchors"""
    return [read[beg:min(beg + WINDOW, len(read) - 1)] for beg in range(0, len(read), STRIDE)]


def planted_overlaps(reads):
    """read pairs (i < j) with at least two pairs of whole windows that hold the same bases and no part of an insert"""
    good = [{w for w in windows_of(r) if len(w) == WINDOW and b"A" * 30 not in w} for r in reads]
    return {(i, j) for i in range(len(reads)) for j in range(i + 1, len(reads)) if len(good[i] & good[j]) >= 2}


def test_reads_with_a_low_complexity_insert(ctx, oracle):
    """Drop the top twentieth of the seeds.  (Checked on the CPU beforehand, with the oracle's bottom-k rows and the brute force
    alone: 63 windows, 21 distinct smallest hashes, the hash of AAA...A in 11 windows, the next ones in 7, 7 and 6; max_occ comes
    out as 7, the mask leaves 158 of 258 window pairs and a window pair for each of the 6 planted overlaps.)"""
    reads = polya_reads()
    planted = planted_overlaps(reads)
    assert len(planted) == 6
    bases, off = oracle.concat(reads)
    params = anchor.AnchorsGeneratorParameters("reads.fasta", WINDOW, NBKMER, K, OVERLAP)
    sp = params.sketch_params(fhash=A.FHASH_CANON_VALUE)
    hashes, _, n, row_off = ctx.read_anchors(bases, off, sp, WINDOW, OVERLAP, want_counts=False)
    group = np.repeat(np.arange(len(reads), dtype=np.uint32), np.diff(row_off.astype(np.int64)))
    n_keys = 1
    with ctx.anchor_index(hashes, n_keys=n_keys, group_db=group) as index:
        top = index.info()["max_occupancy"]
        hist = index.occupancy(top + 1)
    assert top >= len(reads)  # every read has a window of nothing but A
    max_occ = anchor.max_occ_for_fraction(hist, 0.05)
    assert 0 < max_occ < top
    want_p, want_d = brute(oracle, hashes, hashes, n_keys, 1, group, group, max_occ=max_occ)
    plain_p, _ = brute(oracle, hashes, hashes, n_keys, 1, group, group)
    assert 0 < want_p.shape[0] < plain_p.shape[0]
    rec = anchor.match_read_anchors(ctx, hashes, row_off, params, n_keys=n_keys, min_common=1, max_occ=max_occ)
    wa = anchor.rows_to_slices(want_p[:, 0], row_off, STRIDE)
    wb = anchor.rows_to_slices(want_p[:, 1], row_off, STRIDE)
    want = np.stack([wa[0], wa[1], wb[0], wb[1], want_d[:, 0].astype(np.int64), want_d[:, 1].astype(np.int64)], axis=1)
    assert np.array_equal(rec, want)
    assert rec.shape[0] < anchor.match_read_anchors(ctx, hashes, row_off, params, n_keys=n_keys, min_common=1).shape[0]
    ro = anchor.read_overlaps(ctx, hashes, row_off, params, n_keys=n_keys, min_common=1, strands=2, band=1, min_score=2, max_occ=max_occ)
    found = {(int(a), int(b)) for a, b in ro[:, :2].tolist()}
    assert planted <= found
    # the rows on the device: the same records
    import torch
    dh = torch.from_numpy(np.ascontiguousarray(hashes).view(np.int64)).cuda()
    assert np.array_equal(anchor.read_overlaps(ctx, dh, row_off, params, n_keys=n_keys, min_common=1, min_score=2, max_occ=max_occ), ro)

"""Signature comparison (kmu_compare.hip; minhash_walk in kmu_device.h) at the loop, tile and grid edges.

kmu_sig_equal_pairs, kmu_sig_equal_matrix and kmu_minhash_distance_pairs against plain numpy / Python restatements of what
kmu.h promises: rows are compared as raw 4- or 8-byte words, out[p] = #{t : A[ia[p]][t] == B[ib[p]][t]}, the matrix is
out[i * nb + j], the bottom-k walk is minhash.rs:134-190.  Every comparison is an exact integer equality.  Every case runs
from host arrays and from device tensors.  The Python walk is itself pinned to the oracle by the one CPU test of this file."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A

gpu = pytest.mark.gpu

PAD = 0xFFFFFFFFFFFFFFFF  # what fills a bottom-k row behind its entries


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


# ---- the slot values ---------------------------------------------------------------------------------------------------
# Four words per type: WORDS[0] / WORDS[1] differ only in the lowest bit, WORDS[2] / WORDS[3] only in the top half of the word
# (bits 16.. of a 4-byte word, bits 32.. of an 8-byte word).  A compare of half a word takes one of the two pairs for equal.
# The float patterns are ordinary finite numbers (1.0, its successor, 2.0..., -2.0...).
WORDS = {
    "uint32": np.array([0x00010002, 0x00010003, 0x00020007, 0x80030007], np.uint32),
    "uint64": np.array([0x0000000100000002, 0x0000000100000003, 0x0000000200000007, 0x8000000300000007], np.uint64),
    "float32": np.array([0x3F800000, 0x3F800001, 0x40000007, 0xC0010007], np.uint32).view(np.float32),
    "float64": np.array([0x3FF0000000000000, 0x3FF0000000000001, 0x4000000000000007, 0xC000000100000007], np.uint64).view(np.float64),
}
DTYPES = ["uint32", "uint64", "float32", "float64"]


def raw(x):
    """the rows as the unsigned words the library compares"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


def ref_pairs(a, b, ia, ib):
    return (raw(a)[ia] == raw(b)[ib]).sum(-1).astype(np.uint32)


def ref_matrix(a, b):
    return (raw(a)[:, None, :] == raw(b)[None, :, :]).sum(-1).astype(np.uint16)


def to_dev(x):
    """a device tensor with the bits of x (torch has no unsigned 32 / 64-bit tensors: the signed type of the same width)"""
    import torch
    x = np.ascontiguousarray(x)
    if x.dtype.kind == "u":
        x = x.view({2: np.int16, 4: np.int32, 8: np.int64}[x.dtype.itemsize])
    return torch.from_numpy(x.copy()).cuda()


def to_host(ctx, t, dtype):
    ctx.synchronize()
    return t.cpu().numpy().view(dtype)


def pairs_both(ctx, a, b, ia, ib):
    """kmu_sig_equal_pairs from host arrays and from device tensors (a is b stays true on the device)"""
    host = np.asarray(ctx.sig_equal_pairs(a, b, ia, ib))
    ta = to_dev(a)
    tb = ta if b is a else to_dev(b)
    dev = to_host(ctx, ctx.sig_equal_pairs(ta, tb, to_dev(ia), to_dev(ib)), np.uint32)
    return (("host", host), ("device", dev))


def matrix_both(ctx, a, b):
    host = np.asarray(ctx.sig_equal_matrix(a, b))
    ta = to_dev(a)
    tb = ta if b is a else to_dev(b)
    dev = to_host(ctx, ctx.sig_equal_matrix(ta, tb), np.uint16)
    return (("host", host), ("device", dev))


def minhash_both(ctx, a, b, ia, ib):
    host = np.asarray(ctx.minhash_distance_pairs(a, b, ia, ib))
    ta = to_dev(a)
    tb = ta if b is a else to_dev(b)
    dev = to_host(ctx, ctx.minhash_distance_pairs(ta, tb, to_dev(ia), to_dev(ib)), np.uint32)
    return (("host", host), ("device", dev))


def num_cus(ctx):
    """compute units of the device the context runs on: what the library sizes its grids by"""
    import torch
    return int(torch.cuda.get_device_properties(ctx.device_id).multi_processor_count)


# ---- the bottom-k walk -------------------------------------------------------------------------------------------------
def walk(s1, s2):
    """minhash_distance, minhash.rs:134-190, over two ascending lists of Python ints: (common, total, i)"""
    n1, n2 = len(s1), len(s2)
    i = j = common = total = 0
    while i < n1 and j < n2:
        if s1[i] < s2[j]:
            i += 1
        elif s2[j] < s1[i]:
            j += 1
        else:
            i, j, common = i + 1, j + 1, common + 1
        total += 1
        if total >= n1:
            break
    if total < n1:
        if i < n1:
            total += n1 - i
        if j < n1:  # measured against the FIRST list's length, as upstream
            total += n1 - j
        total = min(total, n1)
    return common, total, i


def padded(lists, m):
    rows = np.full((len(lists), m), PAD, np.uint64)
    for r, s in enumerate(lists):
        assert len(s) <= m and all(x < y for x, y in zip(s, s[1:])) and all(x < PAD for x in s)
        rows[r, :len(s)] = np.array(s, np.uint64)
    return rows


H = 1 << 32
HAND_M = 6
HAND_ROWS = [
    [],                                         # 0 empty
    [10, 20, 30, 40, 50, 60],                   # 1 full
    [30],                                       # 2 length 1
    [10, 20, 30],                               # 3, 4 two identical rows, a prefix of row 1
    [10, 20, 30],
    [20, 40, 60],                               # 5 a strict subset of row 1 that is no prefix
    [1, 2, 3, 4],                               # 6 entirely below rows 1..5
    [100, 200, 300, 400, 500],                  # 7 entirely above rows 1..6
    [0, 10, 25, 40],                            # 8 contains 0
    [30, 60, 2 ** 64 - 2],                      # 9 contains the largest hash that is no padding
    [1 * H + 5, 2 * H + 7, 3 * H + 9],          # 10, 11 equal low words, different high words: nothing in common
    [4 * H + 5, 5 * H + 7, 6 * H + 9],
    [5, 15, 30, 45, 50, 70],                    # 12 full, interleaved with row 1: the walk breaks at total == n1 mid-way
]


def random_lists(rng, n, m, pool_size):
    pool = np.arange(1, pool_size + 1, dtype=np.uint64) * np.uint64(0x100000001)  # both halves of the word vary
    lens = rng.integers(0, m + 1, size=n)
    return [np.sort(rng.choice(pool, size=L, replace=False)).tolist() for L in lens]


def walk_table(lists):
    """walk() of every ordered pair of rows: [n, n, 3]"""
    n = len(lists)
    return np.array([[walk(lists[i], lists[j]) for j in range(n)] for i in range(n)], np.uint32).reshape(n, n, 3)


def test_python_walk_matches_oracle(oracle):
    """The reference of the bottom-k tests below is the oracle's: every ordered pair of the hand-made rows, 2 000 random pairs."""
    for s1 in HAND_ROWS:
        for s2 in HAND_ROWS:
            assert walk(s1, s2) == oracle.minhash_distance(np.array(s1, np.uint64), np.array(s2, np.uint64)), (s1, s2)
    rng = np.random.default_rng(17)
    lists = random_lists(rng, 60, 12, 30)
    for i, j in rng.integers(0, len(lists), size=(2000, 2)):
        got = walk(lists[i], lists[j])
        assert got == oracle.minhash_distance(np.array(lists[i], np.uint64), np.array(lists[j], np.uint64)), (lists[i], lists[j])
        # upstream's total is always the first list's length: the loop leaves below n1 only with the second list used up and
        # i < n1, and then the first top-up alone reaches n1 (total >= i).  The second top-up never decides the result.
        assert got[1] == len(lists[i])


# ---- 1. pairs: the 64-slot chunk ---------------------------------------------------------------------------------------
def planted_rows(m):
    """index rows (into WORDS) of pairs with a known count: (a row, b row, count)"""
    rng = np.random.default_rng(1000 + m)
    base = rng.integers(0, 4, size=m)
    out = [(base, base.copy(), m), (base, base ^ 1, 0)]  # identical; every slot differs, each in one half of its word only
    for s in sorted({m - 1, 63, 64}):
        if s < m:
            x, y = base.copy(), base.copy()
            x[s], y[s] = 2, 3  # differ in the top half only
            out.append((x, y, m - 1))
    return out


@gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pairs_chunk_edges(ctx, dtype, m):
    rng = np.random.default_rng(7 * m + len(dtype))
    na, nb = 37, 29
    plant = planted_rows(m)
    a = WORDS[dtype][np.vstack([rng.integers(0, 4, size=(na, m))] + [p[0] for p in plant])]
    b = WORDS[dtype][np.vstack([rng.integers(0, 4, size=(nb, m))] + [p[1] for p in plant])]
    k = len(plant)
    ia = np.concatenate([rng.integers(0, na + k, size=300), na + np.arange(k)]).astype(np.uint32)
    ib = np.concatenate([rng.integers(0, nb + k, size=300), nb + np.arange(k)]).astype(np.uint32)
    want = ref_pairs(a, b, ia, ib)
    assert want[300:].tolist() == [p[2] for p in plant]
    for side, got in pairs_both(ctx, a, b, ia, ib):
        assert np.array_equal(got, want), (side, np.flatnonzero(got != want)[:8])


# ---- 2. pairs: more pairs than waves in the grid -------------------------------------------------------------------------
@gpu
def test_pairs_grid_stride(ctx):
    n_pairs = num_cus(ctx) * 16 * 4 + 77  # the grid is at most 16 workgroups of 4 waves per CU, one pair per wave and turn
    rng = np.random.default_rng(21)
    m, n = 65, 40
    a = WORDS["uint64"][rng.integers(0, 4, size=(n, m))]
    b = WORDS["uint64"][rng.integers(0, 4, size=(n, m))]
    ia = rng.integers(0, n, size=n_pairs).astype(np.uint32)
    ib = rng.integers(0, n, size=n_pairs).astype(np.uint32)
    want = ref_matrix(a, b).astype(np.uint32)[ia, ib]
    assert len(np.unique(want[-77:])) > 1
    for side, got in pairs_both(ctx, a, b, ia, ib):
        assert got.shape == (n_pairs,) and np.array_equal(got, want), (side, np.flatnonzero(got != want)[:8])


# ---- 3. pairs: one array on both sides ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype", ["uint32", "float64"])
def test_pairs_same_array_both_sides(ctx, dtype):
    rng = np.random.default_rng(31)
    n, m = 23, 70
    a = WORDS[dtype][rng.integers(0, 4, size=(n, m))]
    ia = rng.integers(0, n, size=120).astype(np.uint32)
    ib = rng.integers(0, n, size=120).astype(np.uint32)
    ib[:40] = ia[:40]
    want = ref_pairs(a, a, ia, ib)
    assert (want[:40] == m).all() and (want[40:] < m).any()
    for side, got in pairs_both(ctx, a, a, ia, ib):
        assert np.array_equal(got, want), side
    for side, got in matrix_both(ctx, a, a):
        assert np.array_equal(got, ref_matrix(a, a)), side


# ---- 4. matrix: the 64 x 64 tile and the 32-slot chunk ---------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("na,nb", [(1, 1), (1, 65), (63, 64), (64, 64), (65, 63), (129, 1), (130, 67)])
@pytest.mark.parametrize("dtype", ["uint32", "float64"])
def test_matrix_tile_edges(ctx, dtype, na, nb):
    word = np.uint32 if dtype == "uint32" else np.uint64
    for m in (1, 31, 32, 33, 64, 95):
        rng = np.random.default_rng(na * 1000 + nb * 10 + m)
        a = raw(WORDS[dtype][rng.integers(0, 4, size=(na, m))]).copy()
        b = raw(WORDS[dtype][rng.integers(0, 4, size=(nb, m))]).copy()
        # rows of the words the kernel pads with (0 behind a's slots and rows, 1 behind b's), on both sides: a pad that met
        # its like would be counted, a count that is right only because of the pad would not be
        a[0] = 0
        b[0] = 1
        if na > 1:
            a[na - 1] = 1
        if nb > 1:
            b[nb - 1] = 0
        a, b = a.view(word).view(dtype), b.view(word).view(dtype)
        want = ref_matrix(a, b)
        assert want[0, 0] == 0 and (na == 1 or want[na - 1, 0] == m) and (nb == 1 or want[0, nb - 1] == m)
        for side, got in matrix_both(ctx, a, b):
            assert got.shape == (na, nb), (side, m)
            assert np.array_equal(got, want), (side, m, np.argwhere(got != want)[:8].tolist())


# ---- 5. matrix: the range of the 16-bit count ----------------------------------------------------------------------------
@gpu
def test_matrix_count_range(ctx):
    from kmerutils_amd.lib import KmuError
    m = 65535
    rng = np.random.default_rng(51)
    idx = rng.integers(0, 4, size=(2, m))
    a = WORDS["uint32"][idx]
    b = WORDS["uint32"][np.stack([idx[0], idx[1] ^ 1])]  # row 0 equal to a's, row 1 different from a's in every slot
    want = ref_matrix(a, b)
    assert want[0, 0] == 65535 and want[1, 1] == 0 and 0 < want[0, 1] < m
    for side, got in matrix_both(ctx, a, b):
        assert np.array_equal(got, want), (side, got.tolist())
    # one slot more does not fit the count: refused, nothing written
    m = 65536
    a = np.zeros((2, m), np.uint32)
    out = np.full((2, 2), 0x7777, np.uint16)
    rc = ctx.L.kmu_sig_equal_matrix(ctx.h, a.ctypes.data_as(C.c_void_p), 2, a.ctypes.data_as(C.c_void_p), 2, m, A.SIG_U32,
                                    A.MEM_HOST, out.ctypes.data_as(C.c_void_p))
    ctx.synchronize()
    assert rc == A.E_UNSUPPORTED and (out == 0x7777).all()
    ta, tout = to_dev(a), to_dev(out)
    rc = ctx.L.kmu_sig_equal_matrix(ctx.h, C.c_void_p(ta.data_ptr()), 2, C.c_void_p(ta.data_ptr()), 2, m, A.SIG_U32, A.MEM_DEVICE,
                                    C.c_void_p(tout.data_ptr()))
    assert rc == A.E_UNSUPPORTED and (to_host(ctx, tout, np.uint16) == 0x7777).all()
    with pytest.raises(KmuError) as e:
        ctx.sig_equal_matrix(a, a)
    assert e.value.code == A.E_UNSUPPORTED


# ---- 6. bottom-k: hand-made rows ---------------------------------------------------------------------------------------
@gpu
def test_minhash_hand_made_rows(ctx):
    n = len(HAND_ROWS)
    rows = padded(HAND_ROWS, HAND_M)
    ia, ib = [x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(n), np.arange(n), indexing="ij")]
    want = walk_table(HAND_ROWS).reshape(-1, 3)
    tab = want.reshape(n, n, 3)
    # the walk's corners, spelled out
    assert tuple(tab[0, 1]) == (0, 0, 0) and tuple(tab[1, 0]) == (0, 6, 0)      # an empty first row, an empty second row
    assert tuple(tab[1, 1]) == (6, 6, 6) and tuple(tab[3, 4]) == (3, 3, 3)      # a row against itself, against its twin
    assert tuple(tab[3, 1]) == (3, 3, 3) and tuple(tab[1, 3]) == (3, 6, 3)      # a prefix and its superset, both ways
    assert tuple(tab[10, 11]) == (0, 3, 3) and tuple(tab[1, 12]) == (1, 6, 4)   # high words differ; the break mid-way
    for side, got in minhash_both(ctx, rows, rows, ia, ib):
        bad = np.flatnonzero((got != want).any(1))
        assert bad.size == 0, (side, [(int(ia[p]), int(ib[p]), got[p].tolist(), want[p].tolist()) for p in bad[:6]])


@gpu
@pytest.mark.parametrize("m,pool", [(1, 3), (50, 120)])
def test_minhash_random_lengths(ctx, m, pool):
    rng = np.random.default_rng(60 + m)
    lists = random_lists(rng, 30, m, pool)
    lists[0] = []
    lists[1] = ([0] + lists[2])[:m - 1] + [2 ** 64 - 2] if m > 1 else [0]  # the smallest and the largest hash there is
    rows = padded(lists, m)
    ia = rng.integers(0, len(lists), size=400).astype(np.uint32)
    ib = rng.integers(0, len(lists), size=400).astype(np.uint32)
    want = walk_table(lists)[ia, ib]
    for side, got in minhash_both(ctx, rows, rows, ia, ib):
        assert np.array_equal(got, want), (side, np.flatnonzero((got != want).any(1))[:8])


# ---- 7. bottom-k: more pairs than threads in the grid ----------------------------------------------------------------------
@gpu
def test_minhash_grid_stride(ctx):
    n_pairs = num_cus(ctx) * 8 * 256 + 300  # the grid is at most 8 workgroups of 256 threads per CU, one pair per thread and turn
    rng = np.random.default_rng(71)
    m, n = 4, 40
    lists = random_lists(rng, n, m, 9)
    rows_a = padded(lists, m)
    rows_b = padded(lists[::-1], m)
    table = walk_table(lists)[:, ::-1]  # [row of a, row of b]
    ia = rng.integers(0, n, size=n_pairs).astype(np.uint32)
    ib = rng.integers(0, n, size=n_pairs).astype(np.uint32)
    want = table[ia, ib]
    assert len(np.unique(want[-300:], axis=0)) > 4
    for side, got in minhash_both(ctx, rows_a, rows_b, ia, ib):
        assert got.shape == (n_pairs, 3) and np.array_equal(got, want), (side, np.flatnonzero((got != want).any(1))[:8])


# ---- 8. floats are words: signed zeros and NaNs ----------------------------------------------------------------------------
def float_rows(dtype):
    if dtype == "float32":
        u, nz, n1, n2 = np.uint32, 0x80000000, 0x7FC00000, 0xFFC00001
    else:
        u, nz, n1, n2 = np.uint64, 0x8000000000000000, 0x7FF8000000000000, 0xFFF8000000000001
    one, two = np.array([1.5, 2.5], dtype).view(u).tolist()
    rows = np.array([[nz, nz, one, two, nz],     # 0
                     [0, nz, one, two, 0],       # 1: against row 0 three equal words, five equal numbers
                     [n1, n1, one, two, n2],     # 2
                     [n1, n2, one, two, n2]],    # 3: against row 2 four equal words, two equal numbers
                    u)
    return rows.view(dtype), (nz, n1, n2, one)


@gpu
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_rows_are_words(ctx, dtype):
    rows, (nz, n1, n2, one) = float_rows(dtype)
    assert np.isnan(rows[2, 0]) and rows[0, 0] == rows[1, 0] and np.signbit(rows[0, 0])
    want = np.array([[5, 3, 2, 2], [3, 5, 2, 2], [2, 2, 5, 4], [2, 2, 4, 5]], np.uint16)
    assert np.array_equal(ref_matrix(rows, rows), want)
    for side, got in matrix_both(ctx, rows, rows):
        assert np.array_equal(got, want), (side, got.tolist())
    ia, ib = [x.ravel().astype(np.uint32) for x in np.meshgrid(np.arange(4), np.arange(4), indexing="ij")]
    for side, got in pairs_both(ctx, rows, rows, ia, ib):
        assert np.array_equal(got.reshape(4, 4), want), (side, got.tolist())
    # kmu_sig_knn compares "raw words, as above": the nearest row is decided by exactly these slots
    u = raw(rows).dtype
    q = np.array([[nz] * 5, [n1] * 5], u).view(dtype)
    db = np.array([[0] * 5,                     # +0.0 everywhere: five equal numbers, no equal word, for query 0
                   [nz, nz, one, one, one],     # two equal words for query 0
                   [n1, one, one, one, one],    # one equal word for query 1 (no equal number: NaN)
                   [n2] * 5], u).view(dtype)
    for qq, dd in ((q, db), (to_dev(q), to_dev(db))):
        idx, eq = ctx.sig_knn(qq, dd, 1)
        if not isinstance(idx, np.ndarray):
            idx, eq = to_host(ctx, idx, np.uint32), to_host(ctx, eq, np.uint16)
        assert idx.ravel().tolist() == [1, 2] and eq.ravel().tolist() == [2, 1]


# ---- 9. argument rules -------------------------------------------------------------------------------------------------
def p_(x):
    return None if x is None else x.ctypes.data_as(C.c_void_p)


@gpu
def test_argument_rules(ctx):
    from kmerutils_amd.lib import KmuError
    na, nb, m = 5, 4, 9
    rng = np.random.default_rng(91)
    a = WORDS["uint64"][rng.integers(0, 4, size=(na, m))]
    b = WORDS["uint64"][rng.integers(0, 4, size=(nb, m))]
    ia = np.array([0, 4, 2], np.uint32)
    ib = np.array([3, 0, 1], np.uint32)
    out = np.full(3, 0x5A5A5A5A, np.uint32)
    out3 = np.full((3, 3), 0x5A5A5A5A, np.uint32)
    mat = np.full((na, nb), 0x7777, np.uint16)

    def pairs(ia_, ib_, n, m_=m, st=A.SIG_U64):
        return ctx.L.kmu_sig_equal_pairs(ctx.h, p_(a), na, p_(b), nb, m_, st, p_(ia_), p_(ib_), n, A.MEM_HOST, p_(out))

    def walks(ia_, ib_, n, m_=m):
        return ctx.L.kmu_minhash_distance_pairs(ctx.h, p_(a), na, p_(b), nb, m_, p_(ia_), p_(ib_), n, A.MEM_HOST, p_(out3))

    def matrix(na_, nb_, m_=m, st=A.SIG_U64):
        return ctx.L.kmu_sig_equal_matrix(ctx.h, p_(a), na_, p_(b), nb_, m_, st, A.MEM_HOST, p_(mat))

    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        # a host call checks the row indices where it can see them
        bad_a, bad_b = ia.copy(), ib.copy()
        bad_a[2], bad_b[0] = na, nb
        assert pairs(bad_a, ib, 3) == A.E_BAD_ARG and pairs(ia, bad_b, 3) == A.E_BAD_ARG
        assert walks(bad_a, ib, 3) == A.E_BAD_ARG and walks(ia, bad_b, 3) == A.E_BAD_ARG
        with pytest.raises(KmuError) as e:
            ctx.sig_equal_pairs(a, b, bad_a, ib)
        assert e.value.code == A.E_BAD_ARG
        assert pairs(ia, ib, 3, m_=0) == A.E_BAD_ARG and walks(ia, ib, 3, m_=0) == A.E_BAD_ARG and matrix(na, nb, m_=0) == A.E_BAD_ARG
        for st in (-1, A.SIG_U16, 7):
            assert pairs(ia, ib, 3, st=st) == A.E_BAD_ARG and matrix(na, nb, st=st) == A.E_BAD_ARG
        assert pairs(None, ib, 3) == A.E_BAD_ARG and pairs(ia, None, 3) == A.E_BAD_ARG
        # nothing to do is no error: no pairs (the index arrays may be missing), no rows on either side
        assert pairs(None, None, 0) == A.OK and walks(None, None, 0) == A.OK
        assert matrix(0, nb) == A.OK and matrix(na, 0) == A.OK
        ctx.synchronize()
        assert (out == 0x5A5A5A5A).all() and (out3 == 0x5A5A5A5A).all() and (mat == 0x7777).all()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        # the same through the Python layer, host arrays and device tensors
        e32 = np.zeros(0, np.uint32)
        for conv in (lambda x: x, to_dev):
            assert tuple(ctx.sig_equal_pairs(conv(a), conv(b), conv(e32), conv(e32)).shape) == (0,)
            assert tuple(ctx.minhash_distance_pairs(conv(a), conv(b), conv(e32), conv(e32)).shape) == (0, 3)
            assert tuple(ctx.sig_equal_matrix(conv(a[:0]), conv(b)).shape) == (0, nb)
            assert tuple(ctx.sig_equal_matrix(conv(a), conv(b[:0])).shape) == (na, 0)
        ctx.synchronize()
        assert ctx.profile_get() == {}, "an empty call launched a kernel"
        # and the good calls through the same raw path
        assert pairs(ia, ib, 3) == A.OK and np.array_equal(out, ref_pairs(a, b, ia, ib))
        assert matrix(na, nb) == A.OK and np.array_equal(mat, ref_matrix(a, b))
        assert set(ctx.profile_get()) == {"k_sig_equal_pairs", "k_sig_equal_matrix"}
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- 10. the Python layer ----------------------------------------------------------------------------------------------
@gpu
def test_python_layer(ctx):
    from kmerutils_amd import sketching as S
    rng = np.random.default_rng(101)
    n, m = 70, 70
    idx = rng.integers(0, 4, size=(n, m))
    idx[1], idx[2] = idx[0], idx[0] ^ 1  # a twin of row 0, and a row that shares no slot with it
    sig = WORDS["uint64"][idx]
    eq = ref_matrix(sig, sig)
    assert eq[0, 1] == m and eq[0, 2] == 0
    # jaccard_matrix, one argument: every row against every row
    jm = S.jaccard_matrix(sig, ctx=ctx)
    assert jm.shape == (n, n) and np.array_equal(jm, eq.astype(np.float64) / m)
    jd = S.jaccard_matrix(to_dev(sig), ctx=ctx)
    ctx.synchronize()
    # torch divides a device tensor by a scalar as a product with the rounded 1 / m: two roundings of half an ulp each where
    # numpy's division has one, so the quotient is held to two ulps and the count behind it exactly
    jd, want = jd.cpu().numpy(), eq.astype(np.float64) / m
    assert jd.shape == (n, n) and np.array_equal(np.rint(jd * m), eq) and (np.abs(jd - want) <= 2 * np.spacing(want)).all()
    # probminhash_get_jaccard_objects: the jaccard and the objects of the equal slots, None when there is none
    for i, j in [(0, 1), (0, 2), (0, 3), (5, 9), (69, 68), (33, 33)]:
        jp, common = S.probminhash_get_jaccard_objects(sig[i], sig[j], ctx=ctx)
        want = [int(x) for x, y in zip(sig[i].tolist(), sig[j].tolist()) if x == y]
        assert jp == eq[i, j] / m
        assert common == (want if want else None)
    # DistBlockSketched: 1.0 inside a sequence, the fraction of differing slots otherwise
    numseq = np.repeat(np.arange(n // 5), 5).astype(np.uint32)
    ia = rng.integers(0, n, size=300).astype(np.uint32)
    ib = rng.integers(0, n, size=300).astype(np.uint32)
    ia[:3], ib[:3] = [0, 0, 7], [1, 2, 7]
    d = S.DistBlockSketched(ctx).eval_pairs(sig, numseq, ia, ib)
    same = numseq[ia] == numseq[ib]
    want = np.where(same, np.float32(1.0), (np.float32(m) - eq[ia, ib].astype(np.float32)) / np.float32(m))
    assert same.sum() > 3 and (~same).sum() > 200
    assert d.dtype == np.float32 and np.array_equal(d, want)
    # minhash_distance: the fields of MinHashDist
    lists = random_lists(rng, n, 12, 30)
    lists[0] = []
    rows = padded(lists, 12)
    ia[:2], ib[:2] = [0, 1], [1, 0]
    w = walk_table(lists)[ia, ib].astype(np.float64)
    cont, jac, common, total = S.minhash_distance(rows, rows, ia, ib, ctx=ctx)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(cont, w[:, 0] / w[:, 2], equal_nan=True) and np.array_equal(jac, w[:, 0] / w[:, 1], equal_nan=True)
    assert np.array_equal(common, w[:, 0].astype(np.uint64)) and np.array_equal(total, w[:, 1].astype(np.uint64))
    assert np.isnan(jac[0]) and np.isnan(cont[0])  # an empty first row: 0 / 0, as upstream's f64 division

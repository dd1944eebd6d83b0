"""-m gpu: kmu_chain_rank against `reference_rank` (tests/test_chains_all_abi.py: the contract of include/kmu.h in plain Python).
Every case compares whole record arrays exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chains_all_abi import chain_records, reference_rank  # noqa: E402

pytestmark = pytest.mark.gpu
REC = np.dtype(A.CHAIN_DTYPE)
RANK = np.dtype(A.CHAIN_RANK_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def check(ctx, chains, n_reads_q, mask_permille=500):
    want = reference_rank(chains, n_reads_q, mask_permille)
    got = ctx.chain_rank(chains, n_reads_q, mask_permille)
    assert got.dtype == RANK and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "chain %d %s: got %s, want %s" % (bad[0], chains[bad[0]], got[bad[0]], want[bad[0]])
    return got


def random_read(rng, read, n, span=3000, scores=40):
    """n chains of one query read: starts and lengths from small ranges, few different scores -- overlaps and ties everywhere"""
    s = rng.integers(0, span, n)
    return [(read, int(sc), int(a), int(a + ln)) for sc, a, ln in zip(rng.integers(1, scores, n), s, rng.integers(0, 400, n))]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_runs_of_one_read(ctx, n):
    rng = np.random.default_rng(n)
    rows = random_read(rng, 0, n) + random_read(rng, 1, n, span=200 * n) + random_read(rng, 2, 3) + random_read(rng, 3, n, span=100)
    chains = chain_records(rows)
    got = check(ctx, chains, 4)
    for r in range(4):
        of = got[chains["read_a"] == r]
        assert sorted(of["rank"].tolist()) == list(range(of.shape[0]))
    if n >= 63:
        assert (got["parent"] != np.arange(got.shape[0])).any() and (got["n_sub"] > 1).any()
    if n == 129:
        assert (got["parent"][chains["read_a"] == 1] == np.nonzero(chains["read_a"] == 1)[0]).sum() > 64  # primaries beyond one set
    check(ctx, chains, 4, 100)
    check(ctx, chains, 9, 900)


@pytest.mark.parametrize("n", [63, 64, 65, 200])
def test_disjoint_primaries_and_a_secondary_to_the_last(ctx, n):
    # n primaries of 100 bases, 1000 apart, by descending score; then chains inside the last, the first and (n > 70) the 70th
    rows = [(0, 5000 - i, 1000 * i, 1000 * i + 100) for i in range(n)]
    rows += [(0, 7, 1000 * (n - 1) + 10, 1000 * (n - 1) + 60), (0, 6, 20, 90), (0, 5, 1000 * (n - 1), 1000 * (n - 1) + 100)]
    if n > 70:
        rows += [(0, 4, 69000 + 50, 69000 + 150), (0, 3, 69000 + 1, 69000 + 99)]
    chains = chain_records(rows)
    got = check(ctx, chains, 1)
    assert got["parent"][:n].tolist() == list(range(n)) and got["parent"][n:n + 3].tolist() == [n - 1, 0, n - 1]
    assert got[n - 1].tolist() == (n - 1, n - 1, 7, 2) and got[0].tolist() == (0, 0, 6, 1)
    if n > 70:
        assert got["parent"][n + 3:].tolist() == [69, 69] and got[69].tolist() == (69, 69, 4, 2)
    # the same chains in another input order (read_a stays 0): ranks follow the scores, parents the input indices
    perm = np.random.default_rng(n).permutation(chains.shape[0])
    check(ctx, chains[perm], 1)


def test_the_mask_edge(ctx):
    # the shorter chain has 200 bases: at 500 permille an overlap of 100 is enough (100 * 1000 == 500 * 200), 99 is not
    rows = [(0, 90, 0, 1000), (0, 50, 900, 1100), (0, 40, 2000, 2200), (0, 30, 2100, 2300), (0, 20, 4000, 4200), (0, 10, 4101, 4301)]
    chains = chain_records(rows)
    assert check(ctx, chains, 1)["parent"].tolist() == [0, 0, 2, 2, 4, 5]
    assert check(ctx, chains, 1, 501)["parent"].tolist() == [0, 1, 2, 3, 4, 5]
    assert check(ctx, chains, 1, 495)["parent"].tolist() == [0, 0, 2, 2, 4, 4]
    # products beyond 32 bits: an overlap of 2^31 - 1 bases against a chain of as many
    big = chain_records([(0, 9, 0, (1 << 32) - 1), (0, 8, 1 << 31, (1 << 32) - 1), (0, 7, 0, (1 << 31) - 1), (0, 6, (1 << 31) - 2, 1 << 31)])
    assert check(ctx, big, 1, 1000)["parent"].tolist() == [0, 0, 0, 0]


def test_mask_0_and_1000(ctx):
    rows = [(0, 10, 0, 100), (0, 20, 0, 100), (0, 5, 0, 100), (2, 10, 0, 100), (2, 9, 99, 300), (2, 8, 100, 300), (2, 7, 50, 50),
            (2, 6, 10, 90), (2, 5, 10, 101)]
    chains = chain_records(rows)
    assert check(ctx, chains, 3, 0).tolist()[:7] == [(1, 1, 0, 0), (0, 1, 10, 2), (2, 1, 0, 0), (0, 3, 9, 3), (1, 3, 0, 0), (2, 5, 0, 0),
                                                      (3, 6, 0, 0)]
    # 1000: only a chain that lies inside a primary, or holds one, is secondary
    assert check(ctx, chains, 3, 1000)["parent"].tolist() == [1, 1, 1, 3, 4, 4, 6, 3, 8]


def test_equal_scores_fall_back_to_the_input_index(ctx):
    rows = [(0, 7, 0, 100), (0, 9, 50, 150), (0, 9, 60, 160), (0, 7, 500, 600), (1, 3, 0, 10), (1, 3, 0, 10), (1, 3, 0, 10)]
    got = check(ctx, chain_records(rows), 2)
    assert got["rank"].tolist() == [2, 0, 1, 3, 0, 1, 2] and got["parent"].tolist() == [1, 1, 1, 3, 4, 4, 4]
    assert got[4].tolist() == (0, 4, 3, 2)
    rng = np.random.default_rng(3)
    chains = chain_records(random_read(rng, 0, 300, span=500, scores=3))  # three different scores among 300 chains
    check(ctx, chains, 1)


def test_reads_without_chains_between_reads_that_have_them(ctx):
    rng = np.random.default_rng(4)
    rows = []
    for read in (3, 4, 700, 701, 99999):
        rows += random_read(rng, read, 20)
    chains = chain_records(rows)
    check(ctx, chains, 100000)
    check(ctx, chains[20:40], 5)      # only the last read has chains
    check(ctx, chains[:20], 100000)   # only an early one


def test_many_reads(ctx):
    rng = np.random.default_rng(5)
    rows = []
    for read in range(6000):  # more reads than one grid pass
        rows += random_read(rng, read, int(rng.integers(0, 4)), span=300)
    check(ctx, chain_records(rows), 6000)


def raw(ctx, chains, n, n_reads_q, p, out, mem=A.MEM_HOST):
    ptr = lambda x: None if x is None else lib._ptr(x)[0]  # noqa: E731
    return ctx.L.kmu_chain_rank(ctx.h, ptr(chains), n, n_reads_q, None if p is None else C.byref(p), mem, ptr(out))


def test_refusals(ctx):
    rng = np.random.default_rng(6)
    chains = chain_records(random_read(rng, 0, 30) + random_read(rng, 2, 30))
    want = reference_rank(chains, 3)
    out = np.zeros(60, RANK)
    uns, bad = A.E_UNSUPPORTED, A.E_BAD_ARG
    assert raw(ctx, chains, 60, 2, A.RankParams(500, 0), out) == uns   # read_a >= n_reads_q
    swapped = chains.copy()
    swapped[[0, 59]] = swapped[[59, 0]]
    assert raw(ctx, swapped, 60, 3, A.RankParams(500, 0), out) == uns  # read_a falls
    back = chains.copy()
    back["a_start"][17], back["a_end"][17] = 900, 899
    assert raw(ctx, back, 60, 3, A.RankParams(500, 0), out) == uns     # a start behind its end
    with pytest.raises(lib.KmuError) as e:
        ctx.chain_rank(back, 3)
    assert e.value.code == uns
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out[:] = (9, 9, 9, 9)
        assert raw(ctx, chains, 60, 3, A.RankParams(1001, 0), out) == bad
        assert raw(ctx, chains, 60, 3, A.RankParams(500, 1), out) == bad
        assert raw(ctx, None, 60, 3, A.RankParams(500, 0), out) == bad
        assert raw(ctx, chains, 60, 3, None, out) == bad
        assert raw(ctx, chains, 60, 3, A.RankParams(500, 0), None) == bad
        assert raw(ctx, chains, 60, 3, A.RankParams(500, 0), out, mem=7) == bad
        assert raw(ctx, chains, 60, 0, A.RankParams(500, 0), out) == bad
        assert raw(ctx, chains, 1 << 32, 3, A.RankParams(500, 0), out) == uns
        assert raw(ctx, chains, 0, 3, A.RankParams(500, 0), out) == A.OK
        assert out.tolist() == [(9, 9, 9, 9)] * 60
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        assert raw(ctx, chains, 60, 3, A.RankParams(500, 0), out) == A.OK and np.array_equal(out, want)  # the context still works
        prof = ctx.profile_get()
        for name in ("k_rank_keys", "k_sort_scatter", "k_rank_starts", "k_rank_walk"):
            assert name in prof, name
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    assert ctx.chain_rank(chains[:0], 3).shape == (0,)


def test_device_tensors_give_the_same_records(ctx):
    import torch
    rng = np.random.default_rng(7)
    rows = []
    for read in range(40):
        rows += random_read(rng, read, int(rng.integers(0, 90)))
    chains = chain_records(rows)
    for mask in (0, 500, 1000):
        want = check(ctx, chains, 40, mask)
        got = ctx.chain_rank(torch.from_numpy(chains.view(np.int32).reshape(-1, 10)).cuda(), 40, mask)
        assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (chains.shape[0], 4)
        assert got.cpu().numpy().tobytes() == want.tobytes()
    back = chains.copy()
    back["read_a"][5] = 41
    with pytest.raises(lib.KmuError) as e:  # found on the device, refused at the call's synchronisation
        ctx.chain_rank(torch.from_numpy(back.view(np.int32).reshape(-1, 10)).cuda(), 40)
    assert e.value.code == A.E_UNSUPPORTED

"""kmu_read_stats on the device against tests/read_stats_model.py, exact equality, at the smallest shapes where its kernels can go
wrong: reads around a lane's 16 bytes and a wave step's 1024, runs of empty reads and many reads per 16 bytes (the slow path), a
read of many 16 KiB regions (the fast path), a batch that is a range of a larger one, bytes of every kind, the rounding ties, the
joins of the length buckets and the end of the histogram, host and device memory, every combination of optional outputs, and the
call's ownership of its outputs."""
import itertools
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_stats_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
COMP = np.dtype(A.READ_COMP_DTYPE)
LETTERS = np.frombuffer(b"ACGTacgtNn\n\x00\xff", np.uint8)
WEIGHTS = np.array([20, 20, 20, 20, 3, 3, 3, 3, 2, 2, 1, 1, 2], np.float64) / 100


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context()
    yield c
    c.close()


def batch(lengths, seed, letters=LETTERS, weights=WEIGHTS):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    return rng.choice(letters, int(off[-1]), p=weights), off


def on_device(x):
    import torch
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    pad = np.zeros(x.size + 64, x.dtype)  # (room behind the last base: an aligned 16-byte load may reach past it)
    pad[:x.size] = x
    return torch.from_numpy(pad).cuda()[:x.size]


def to_host(comp, pct, hist):
    return (None if comp is None else comp.cpu().numpy().view(COMP).reshape(-1),
            None if pct is None else pct.cpu().numpy().view(np.uint64), None if hist is None else hist.cpu().numpy().view(np.uint64))


def same(got, want, what=""):
    comp, pct, hist, info = got
    w_comp, w_pct, w_hist, w_info = want
    assert info == w_info, what
    if comp is not None:
        for name in COMP.names:
            assert np.array_equal(comp[name], w_comp[name]), (what, name)
    if pct is not None:
        assert np.array_equal(pct, w_pct) and int(pct.sum()) == 4 * w_info["n_reads"], what
    if hist is not None:
        assert np.array_equal(hist, w_hist), what


def run_both(ctx, bases, off, **kw):
    """host call and device call, both against the model"""
    want = M.read_stats(bases, off, **kw)
    same(ctx.read_stats(bases, off, **kw), want, "host")
    comp, pct, hist, info = ctx.read_stats(on_device(bases), on_device(off), **kw)
    same(to_host(comp, pct, hist) + (info,), want, "device")
    return want


EDGE_LENGTHS = [0, 1, 15, 16, 17, 1023, 1024, 1025]


def test_no_reads(ctx):
    want = run_both(ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert want[3]["n_reads"] == 0 and want[3]["min_len"] == 0 and want[3]["n_buckets"] == 11264


@pytest.mark.parametrize("length", EDGE_LENGTHS)
def test_one_read(ctx, length):
    bases, off = batch([length], 100 + length)
    want = run_both(ctx, bases, off)
    assert want[3]["n_empty"] == (length == 0) and want[3]["min_len"] == want[3]["max_len"] == length


def test_edge_lengths_in_one_batch(ctx):
    bases, off = batch(EDGE_LENGTHS + EDGE_LENGTHS[::-1], 7)
    run_both(ctx, bases, off)


def test_many_short_reads_with_runs_of_empty_ones(ctx):
    rng = np.random.default_rng(11)
    lengths = rng.integers(0, 41, 3000)
    lengths[[0, 1, 2, 500, 501, 502, 503, 2998, 2999]] = 0  # an empty first and last read, runs of empty reads
    lengths[1000:1040] = rng.integers(0, 3, 40)             # many reads inside one lane's 16 bytes
    bases, off = batch(lengths, 12)
    want = run_both(ctx, bases, off)
    assert want[3]["n_empty"] >= 9 and int(want[1][0].sum()) >= 4 * want[3]["n_empty"]  # empty reads land in row 0


@pytest.mark.parametrize("around", [False, True], ids=["alone", "between_short_reads"])
def test_long_read_over_many_regions(ctx, around):
    lengths = [200_000] if not around else [3, 0, 700, 200_000, 0, 5, 1024, 33]
    bases, off = batch(lengths, 21 + around)
    want = run_both(ctx, bases, off)
    assert want[3]["max_len"] == 200_000


@pytest.mark.parametrize("first", [5, 1029])
def test_a_range_of_a_larger_batch(ctx, first):
    """offsets[0] = first: the bytes in front of it belong to no read and are counted nowhere"""
    lengths = [first, 40, 0, 1500, 17, 20_000, 1]
    bases, off = batch(lengths, 31 + first)
    sub = off[1:]
    assert int(sub[0]) == first
    want = M.read_stats(bases, sub)
    same(ctx.read_stats(bases, sub), want, "host")
    comp, pct, hist, info = ctx.read_stats(on_device(bases), on_device(off)[1:])
    same(to_host(comp, pct, hist) + (info,), want, "device")
    assert want[3]["n_bases"] == int(off[-1]) - first


def test_bytes_of_every_kind(ctx):
    bases = np.concatenate([np.arange(256, dtype=np.uint8), np.frombuffer(b"acgtACGTNn\n\x00\xff", np.uint8)])
    off = np.array([0, 256, 260, 264, bases.size], np.uint64)
    want = run_both(ctx, bases, off)
    assert want[0]["n_base"][0].tolist() == [2, 2, 2, 2] and want[0]["n_other"][0] == 248 and want[3]["n_other"] == 248 + 5


def test_rounding_ties_and_the_extreme_rows(ctx):
    reads = [b"A" + b"C" * 7, b"A" + b"C" * 199, b"A" + b"C" * 39, b"A" * 50, b"CGT" * 10]
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.uint64)
    want = run_both(ctx, bases, off)
    assert want[0]["pct"][:, 0].tolist() == [13, 1, 3, 100, 0]
    assert want[1][100, 0] == 1 and want[1][0, 0] == 1  # an all-A read in row 100, a read without A in row 0


def test_the_joins_of_the_length_buckets(ctx):
    lengths = [2047, 2048, 2049, 4095, 4096]
    bases, off = batch(lengths, 41, LETTERS[:4], np.full(4, .25))
    want = run_both(ctx, bases, off, max_len=5000, sig_digits=3)
    assert want[0]["len_bucket"].tolist() == [2047, 2048, 2048, 3071, 3072] and want[3]["n_buckets"] == 4096 and want[3]["histo_out"] == 0


def test_the_end_of_the_histogram(ctx):
    lengths = [31, 32, 33, 63, 64, 65]
    bases, off = batch(lengths, 42)
    want = run_both(ctx, bases, off, max_len=63, sig_digits=1)
    assert want[0]["len_bucket"].tolist() == [31, 32, 32, 47, M.NO_BUCKET, M.NO_BUCKET]
    assert want[3]["histo_out"] == 2 and want[3]["n_buckets"] == 48 and int(want[2].sum()) == 4


def test_one_length_is_one_bucket(ctx):
    bases, off = batch([150] * 5000, 43)
    want = run_both(ctx, bases, off)
    assert want[2][150] == 5000 and int(want[2].sum()) == 5000


def test_optional_outputs_and_ownership_of_the_outputs(ctx):
    import torch
    bases, off = batch([0, 40, 1500, 17, 20_000, 1, 0], 51)
    want = M.read_stats(bases, off)
    d_bases, d_off = on_device(bases), on_device(off)
    for names in itertools.chain.from_iterable(itertools.combinations(("comp", "pct", "len"), k) for k in range(4)):
        for args in ((bases, off), (d_bases, d_off)):
            comp, pct, hist, info = ctx.read_stats(*args, want=names)
            assert [x is not None for x in (comp, pct, hist)] == [n in names for n in ("comp", "pct", "len")]
            if args[0] is d_bases:
                comp, pct, hist = to_host(comp, pct, hist)
            same((comp, pct, hist, info), want, str(names))
    # device outputs that hold 0xFF on entry are overwritten, and a second call into the same buffers gives the same values
    into = (torch.full((off.size - 1, 12), -1, dtype=torch.int32, device="cuda"), torch.full((101, 4), -1, dtype=torch.int64, device="cuda"),
            torch.full((11264,), -1, dtype=torch.int64, device="cuda"))
    for _ in range(2):
        comp, pct, hist, info = ctx.read_stats(d_bases, d_off, into=into)
        same(to_host(comp, pct, hist) + (info,), want, "into")
    host_into = (np.full(off.size - 1, 0xFF, np.uint8).repeat(48).view(COMP), np.full((101, 4), 7, np.uint64), np.full(11264, 7, np.uint64))
    for _ in range(2):
        same(ctx.read_stats(bases, off, into=host_into), want, "host into")


def test_bad_parameters_write_nothing(ctx):
    """the C call itself, below the binding (whose layout call would refuse first): host and device outputs keep what they held"""
    import ctypes as C
    import torch
    from kmerutils_amd import lib
    bases, off = batch([40, 17], 61)
    comp, pct, hist = np.full(2 * 48, 7, np.uint8), np.full((101, 4), 7, np.uint64), np.full(11264, 7, np.uint64)
    d_bases, d_off = on_device(bases), on_device(off)
    d_comp, d_pct, d_hist = (torch.full((n,), 7, dtype=torch.int64, device="cuda") for n in (12, 404, 11264))
    for sig_digits, flags, max_len in ((0, 0, 1000), (6, 0, 1000), (-1, 0, 1000), (3, 0, 0), (3, 1, 1000)):
        p = A.ReadStatsParams(sig_digits, flags, max_len)
        for mem, args, outs in ((A.MEM_HOST, (bases, off), (comp, pct, hist)), (A.MEM_DEVICE, (d_bases, d_off), (d_comp, d_pct, d_hist))):
            info = A.ReadStatsInfo()
            info.n_reads = 7
            rc = ctx.L.kmu_read_stats(ctx.h, C.byref(p), lib._ptr(args[0])[0], lib._ptr(args[1])[0], 2, mem, *(lib._ptr(x)[0] for x in outs), C.byref(info))
            assert rc == A.E_BAD_ARG and info.n_reads == 7, (sig_digits, flags, max_len, mem)
            assert all(bool((x == 7).all()) for x in outs), (sig_digits, flags, max_len, mem)
    with pytest.raises(lib.KmuError) as e:  # (and the binding reports the same code)
        ctx.read_stats(bases, off, sig_digits=6)
    assert e.value.code == A.E_BAD_ARG

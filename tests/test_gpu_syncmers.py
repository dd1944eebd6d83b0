"""-m gpu: kmu_read_syncmers against `reference_syncmers` (tests/test_syncmers_abi.py: the rule of include/kmu.h as plain numpy,
checked there against a brute force) over the oracle's kmer_hashes for the s-mers and for the k-mers.  The strand reference is that
of tests/test_gpu_minimizers.py::expected, taken at w = 1 (every k-mer) and looked up at the selected positions.  Every case
compares whole arrays exactly, the offsets included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_minimizers import NTHASH, expected, host, rand_reads, revcomp, same  # noqa: E402
from test_syncmers_abi import reference_syncmers  # noqa: E402

pytestmark = pytest.mark.gpu
T = A.SYNCMER_TILE
INV = A.FHASH_CANON_INVHASH


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def expected_sync(oracle, bases, off, kmer_type, k, fhash, s, t, s_fhash=None, s_kmer_type=None, h=None, every=None):
    """(hashes, pos, read, strand or None, sync_offsets) of the reads bases[off[0] : off[-1]].  h and every: the k-mer hashes and
    the w = 1 result of test_gpu_minimizers.expected for the same reads, for callers that walk several (s, t)."""
    off = np.asarray(off, np.uint64)
    sub = np.ascontiguousarray(bases[int(off[0]):max(int(off[-1]), int(off[0]) + 1)])
    off0 = off - off[0]
    if h is None:
        h = oracle.kmer_hashes(sub, off0, kmer_type, k, fhash)
    g = oracle.kmer_hashes(sub, off0, A.kmer_type_for_k(s) if s_kmer_type is None else s_kmer_type, s, fhash if s_fhash is None else s_fhash)
    hashes, pos, read, soff = reference_syncmers(g, h, off0, k, s, t)
    strand = None
    if fhash not in NTHASH:
        if every is None:
            every = expected(oracle, sub, off0, kmer_type, k, fhash, 1, h)
        first = every[4].astype(np.int64)  # w = 1: entry first[i] + p is position p of read i
        strand = every[3][first[read.astype(np.int64)] + pos.astype(np.int64)]
    return hashes, pos, read, strand, soff


def run(ctx, bases, off, kmer_type, k, fhash, s, t, s_fhash=None, s_kmer_type=None):
    return ctx.read_syncmers(bases, off, kmer_type, k, fhash, s, t, s_kmer_type, s_fhash,
                             want=("pos", "read") if fhash in NTHASH else lib.MINIMIZERS_WANT)


def check(ctx, oracle, reads, kmer_type, k, fhash, s, t, **kw):
    bases, off = oracle.concat(reads)
    want = expected_sync(oracle, bases, off, kmer_type, k, fhash, s, t, **kw)
    got = run(ctx, bases, off, kmer_type, k, fhash, s, t, kw.get("s_fhash"), kw.get("s_kmer_type"))
    same(got, want, "k %d s %d t %d" % (k, s, t))
    return [host(g) for g in got]


# ---- parity ---------------------------------------------------------------------------------------------------------------------
OTHER_S = {11: 8, 16: 15, 21: 11, 31: 11}  # 16 -> 15 and 21, 31 -> 11: the s-mers in another integer width than the k-mers


@pytest.mark.parametrize("fhash", [INV, A.FHASH_CANON_VALUE, A.FHASH_VALUE_MASKED, A.FHASH_CANON_NTHASH],
                         ids=["canon_invhash", "canon_value", "value_masked", "canon_nthash"])
@pytest.mark.parametrize("kmer_type,k", [(A.KMER32BIT, 11), (A.KMER16B32BIT, 16), (A.KMER64BIT, 21), (A.KMER64BIT, 31)])
def test_parity(ctx, oracle, kmer_type, k, fhash):
    lens = np.random.default_rng(k).integers(1, 3001, size=40)
    reads = rand_reads(200 + k, lens)
    bases, off = oracle.concat(reads)
    h = oracle.kmer_hashes(bases, off, kmer_type, k, fhash)
    every = None if fhash in NTHASH else expected(oracle, bases, off, kmer_type, k, fhash, 1, h)
    assert A.kmer_type_for_k(OTHER_S[k]) != kmer_type or k == 11
    for s in (1, 5, OTHER_S[k], k):
        u = k - s
        for t in sorted({0, u // 4, u // 2}):
            want = expected_sync(oracle, bases, off, kmer_type, k, fhash, s, t, h=h, every=every)
            same(run(ctx, bases, off, kmer_type, k, fhash, s, t), want, "k %d s %d t %d" % (k, s, t))
            if s == k:  # every k-mer
                assert np.array_equal(want[1], np.concatenate([np.arange(max(0, int(n) - k + 1)) for n in lens]))


@pytest.mark.parametrize("fhash,s_fhash", [(INV, A.FHASH_CANON_NTHASH), (A.FHASH_VALUE_MASKED, A.FHASH_CANON_VALUE), (A.FHASH_CANON_NTHASH, INV)],
                         ids=["invhash_by_nthash", "masked_by_canon_value", "nthash_by_invhash"])
def test_the_s_mers_under_another_order_than_the_k_mers(ctx, oracle, fhash, s_fhash):
    reads = rand_reads(31, [2500, 40, 1300, 3 * T + 9])
    got = check(ctx, oracle, reads, A.KMER64BIT, 21, fhash, 11, 2, s_fhash=s_fhash)
    assert 0 < got[0].size < sum(len(r) for r in reads)
    # the strand belongs to the k-mers' order: an ntHash order of the s-mers leaves it in place
    assert (got[3] is None) == (fhash in NTHASH)


# ---- tiles and steps --------------------------------------------------------------------------------------------------------------
EDGE_NK = (1, 2, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 3)


@pytest.mark.parametrize("s,t", [(11, 0), (11, 5), (1, 0), (1, 10), (1, 4)])
def test_tile_boundaries(ctx, oracle, s, t):
    """s = 1: the widest reach behind a tile at this k (u = 20), and four values of g: ties everywhere"""
    k = 21
    lens = [nk + k - 1 for nk in EDGE_NK]
    got = check(ctx, oracle, rand_reads(40 + s, lens), A.KMER64BIT, k, INV, s, t)
    n = np.diff(got[4].astype(np.int64))
    assert (n <= EDGE_NK).all() and n[-1] > 0


def test_tile_boundaries_behind_every_word_lead(ctx, oracle):
    """the same reads behind a first read of 1 .. 17 bases: the place of a read's first base in its 16-base word differs"""
    k = 21
    reads = rand_reads(50, [nk + k - 1 for nk in EDGE_NK])
    modes = [(11, 0), (1, 10), (11, 5), (1, 0)]
    for lead in range(1, 18):
        s, t = modes[lead % 4]
        check(ctx, oracle, rand_reads(60 + lead, [lead]) + reads, A.KMER64BIT, k, INV, s, t)


def test_batch_that_starts_inside_a_larger_array(ctx, oracle):
    import torch
    k, s, t = 21, 11, 0
    reads = rand_reads(9, [333, 700, 41, 1200, 515, 90, 0, 20, 2500])
    bases, off = oracle.concat(reads)
    first, last = 2, 6
    want = expected_sync(oracle, bases, off[first:last + 1], A.KMER64BIT, k, INV, s, t)
    same(run(ctx, bases, off[first:last + 1].copy(), A.KMER64BIT, k, INV, s, t), want, "host")
    d_bases = torch.from_numpy(bases).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    same(run(ctx, d_bases, d_off[first:last + 1], A.KMER64BIT, k, INV, s, t), want, "device")


def test_more_tiles_than_workgroups(ctx, oracle):
    """the driver launches at most 40 workgroups per CU: one tile more than that, so that the grid-stride loop takes a second trip"""
    import torch
    k = 21
    n = 40 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    lens = np.random.default_rng(16).integers(k, k + 6, size=n)
    got = check(ctx, oracle, rand_reads(17, lens), A.KMER64BIT, k, INV, 11, 0)
    per_read = np.diff(got[4].astype(np.int64))
    assert per_read.size == n and (per_read <= lens - k + 1).all() and per_read[-1000:].sum() > 0  # the last tiles were taken too


def test_more_tiles_than_a_fresh_workspace_holds(oracle):
    """A device call does not know its number of tiles: it counts into the workspace the context has (65 536 tiles in a fresh one)
    and counts again when they did not fit.  65 537 reads of k bases are 65 537 tiles; then a small batch on the grown workspace,
    whose entries behind the last tile must count as nothing."""
    import torch
    k, s, t = 21, 11, 5
    reads = rand_reads(18, [k] * 65537)
    bases, off = oracle.concat(reads)
    want = expected_sync(oracle, bases, off, A.KMER64BIT, k, INV, s, t)
    c = lib.Context(0)
    try:
        d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
        got = run(c, d_bases, d_off, A.KMER64BIT, k, INV, s, t)
        assert all(x.is_cuda for x in got)
        same(got, want, "fresh")
        few = expected_sync(oracle, bases, off[:8], A.KMER64BIT, k, INV, s, t)
        same(run(c, d_bases, d_off[:8].clone(), A.KMER64BIT, k, INV, s, t), few, "grown")
    finally:
        c.close()


# ---- degenerate reads ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fhash", [A.FHASH_CANON_VALUE, A.FHASH_VALUE_MASKED, INV], ids=["canon_value", "value_masked", "canon_invhash"])
def test_one_base_repeated_and_period_two(ctx, oracle, fhash):
    k = 21
    for s, t in ((11, 0), (11, 3), (11, 5), (1, 0)):
        got = check(ctx, oracle, [b"A" * 2500, b"T" * 1100], A.KMER64BIT, k, fhash, s, t)
        assert np.array_equal(got[1], np.concatenate([np.arange(2500 - k + 1), np.arange(1100 - k + 1)]))  # every k-mer
        want_strand = [0] * (2500 - k + 1) + [int(fhash != A.FHASH_VALUE_MASKED)] * (1100 - k + 1)  # poly-T: its reverse complement is poly-A
        assert got[3].tolist() == want_strand
        check(ctx, oracle, [b"AC" * 1300, b"ACGT" * 600], A.KMER64BIT, k, fhash, s, t)


def test_palindromic_k_mers_have_strand_0(ctx, oracle):
    k = 20
    read = b"ACGT" * 300  # the 20-mers at 0 mod 4 are their own reverse complement
    for s, t in ((20, 0), (8, 0), (8, 6)):
        got = check(ctx, oracle, [read, rand_reads(70, [500])[0]], A.KMER64BIT, k, INV, s, t)
        own = got[1][:int(got[4][1])]
        pal = own % 4 == 0
        assert (pal.any() or s < k) and (got[3][:own.size][pal] == 0).all()


def test_empty_and_short_reads_between_real_ones(ctx, oracle):
    k, s = 21, 11
    lens = [0, 500, 1, s - 1, s, 0, k - 1, T + k + 5, 20, 0, k, 3]
    got = check(ctx, oracle, rand_reads(71, lens), A.KMER64BIT, k, INV, s, 0)
    n = np.diff(got[4].astype(np.int64))
    assert all(x <= max(0, L - k + 1) for x, L in zip(n.tolist(), lens)) and n[1] > 0 and n[7] > 0
    got = ctx.read_syncmers(np.frombuffer(b"ACGTACGTAC" + b"A" * 6, np.uint8).copy(), np.array([0, 4, 4, 10], np.uint64), A.KMER64BIT, k, INV, s)
    assert got[0].size == 0 and got[4].tolist() == [0, 0, 0, 0]


def test_a_batch_of_empty_reads_on_host_and_device_arrays(ctx):
    import torch
    off = np.zeros(4, np.uint64)
    got = ctx.read_syncmers(np.zeros(0, np.uint8), off, A.KMER64BIT, 21, INV, 11)
    assert [x.shape for x in got] == [(0,)] * 4 + [(4,)] and got[4].tolist() == [0, 0, 0, 0]
    d = ctx.read_syncmers(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), A.KMER64BIT, 21, INV, 11)
    assert all(x.is_cuda for x in d) and [tuple(x.shape) for x in d] == [(0,)] * 4 + [(4,)] and d[4].cpu().tolist() == [0, 0, 0, 0]


# ---- the mirror property ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 2, 5])
def test_reverse_complement_gives_mirrored_seeds(ctx, oracle, t):
    k, s = 21, 11
    lens = np.random.default_rng(80).integers(k, 2 * T + 200, size=20)
    reads = rand_reads(81, lens)
    bases, off = oracle.concat(reads)
    fw = [host(x) for x in ctx.read_syncmers(bases, off, A.KMER64BIT, k, INV, s, t)]
    bases_rc, _ = oracle.concat([revcomp(r) for r in reads])
    rc = [host(x) for x in ctx.read_syncmers(bases_rc, off, A.KMER64BIT, k, INV, s, t)]
    assert np.array_equal(fw[4], rc[4]) and fw[0].size > 0
    for i, r in enumerate(reads):
        b, e = int(fw[4][i]), int(fw[4][i + 1])
        assert np.array_equal(rc[1][b:e][::-1], len(r) - k - fw[1][b:e])  # nk - 1 - p
        assert np.array_equal(rc[0][b:e][::-1], fw[0][b:e])               # the same hashes
        assert np.array_equal(rc[3][b:e][::-1], 1 - fw[3][b:e])           # k is odd: no k-mer is its own reverse complement


# ---- buffers and calls ----------------------------------------------------------------------------------------------------------------
BATCH = dict(kmer_type=A.KMER64BIT, k=21, fhash=INV, s=11, t=0)


@pytest.fixture(scope="module")
def batch(oracle):
    reads = rand_reads(9, [333, 700, 41, 1200, 515, 90, 0, 20, 2500])
    bases, off = oracle.concat(reads)
    return bases, off, expected_sync(oracle, bases, off, **BATCH)


def raw(ctx, bases, off, hashes, pos, read, strand, cap, soff, mem=A.MEM_HOST, kmer_type=None, k=None, fhash=None, input_kind=A.INPUT_ASCII,
        s=None, t=None, s_kmer_type=None, s_fhash=None):
    """kmu_read_syncmers through the raw C-ABI: (status, *n_out)"""
    hp = A.HashParams(BATCH["kmer_type"] if kmer_type is None else kmer_type, BATCH["k"] if k is None else k,
                      BATCH["fhash"] if fhash is None else fhash, input_kind, mem, 0)
    s = BATCH["s"] if s is None else s
    sp = A.SyncmerParams(A.kmer_type_for_k(s) if s_kmer_type is None else s_kmer_type, s, BATCH["fhash"] if s_fhash is None else s_fhash,
                         BATCH["t"] if t is None else t)
    total = C.c_uint64(0xDEAD)
    P = lambda x: lib._ptr(x)[0]  # noqa: E731
    rc = ctx.L.kmu_read_syncmers(ctx.h, C.byref(hp), C.byref(sp), P(bases), P(off), len(off) - 1, P(hashes), P(pos), P(read), P(strand), cap,
                                 P(soff), C.byref(total))
    return rc, int(total.value)


def test_count_only_call_writes_nothing_else(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    pos, read, strand = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5, np.uint8)
    soff = np.full(off.size, 77, np.uint64)
    assert raw(ctx, bases, off, None, pos, read, strand, n, soff) == (A.OK, n)
    assert (pos == 0xA5A5A5A5).all() and (read == 0xA5A5A5A5).all() and (strand == 0xA5).all()
    assert np.array_equal(soff, want[4])
    assert raw(ctx, bases, off, None, None, None, None, 0, None) == (A.OK, n)


def test_cap_rules(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    out = [np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(off.size, np.uint64)]
    assert raw(ctx, bases, off, out[0], out[1], out[2], out[3], n, out[4]) == (A.OK, n)  # the written total is the counted one
    same(out, want)
    assert raw(ctx, bases, off, out[0], None, None, None, n - 1, None) == (A.E_BAD_ARG, n)
    # the number of k-mers, with no count-only call in front
    cap = int(lib.minimizer_layout(off, BATCH["k"], 1)[-1])
    assert cap == sum(max(0, int(x) - BATCH["k"] + 1) for x in np.diff(off.astype(np.int64))) and cap > n
    out = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(off.size, np.uint64)]
    assert raw(ctx, bases, off, out[0], out[1], out[2], out[3], cap, out[4]) == (A.OK, n)
    same([x[:n] for x in out[:4]] + [out[4]], want)
    # s == k fills that capacity exactly
    full = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint32)]
    assert raw(ctx, bases, off, full[0], full[1], None, None, cap, None, s=BATCH["k"], s_kmer_type=A.KMER64BIT) == (A.OK, cap)


def test_numpy_in_numpy_out_torch_in_torch_out(ctx, batch):
    import torch
    bases, off, want = batch
    got = ctx.read_syncmers(bases, off, BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["s"], BATCH["t"])
    assert all(isinstance(x, np.ndarray) for x in got)
    assert [x.dtype for x in got] == [np.uint64, np.uint32, np.uint32, np.uint8, np.uint64]
    same(got, want)
    dev = ctx.read_syncmers(torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), BATCH["kmer_type"], BATCH["k"],
                            BATCH["fhash"], BATCH["s"], BATCH["t"])
    assert all(x.is_cuda for x in dev)
    assert [x.dtype for x in dev] == [torch.int64, torch.int32, torch.int32, torch.uint8, torch.int64]
    same(dev, want)
    same(dev, got)
    rec = minimizer.read_syncmers(ctx, bases, off, BATCH["k"], BATCH["s"], BATCH["t"])
    assert (rec.k, rec.s, rec.t, rec.fhash) == (21, 11, 0, INV)
    same(rec[:5], want)
    assert minimizer.read_syncmers(ctx, bases, off, 21, 11, 2, fhash=A.FHASH_CANON_NTHASH).strand is None


def test_two_calls_give_identical_arrays(ctx, oracle):
    bases, off = oracle.concat(rand_reads(10, [5 * T + 17, 40, 900]))
    same(ctx.read_syncmers(bases, off, A.KMER64BIT, 21, INV, 11, 3), ctx.read_syncmers(bases, off, A.KMER64BIT, 21, INV, 11, 3))


# ---- errors -------------------------------------------------------------------------------------------------------------------------
def test_non_acgt_is_reported_and_does_not_stick(ctx, oracle):
    k, s = 21, 11
    reads = rand_reads(12, [400, 2 * T + 300, 15])
    spots = [(0, 100), (1, T + 50 + k - 1), (1, len(reads[1]) - 1), (2, 3), (2, 14), (0, 0)]  # the last base of a long read; a read shorter than k
    for r, p in spots:
        bad = [bytearray(x) for x in reads]
        bad[r][p] = ord("N")
        bases, off = oracle.concat([bytes(x) for x in bad])
        with pytest.raises(lib.KmuError) as e:
            ctx.read_syncmers(bases, off, A.KMER64BIT, k, INV, s)
        assert e.value.code == A.E_NON_ACGT, (r, p)
        assert raw(ctx, bases, off, None, None, None, None, 0, None)[0] == A.E_NON_ACGT
        check(ctx, oracle, reads, A.KMER64BIT, k, INV, s, 0)  # the next call is clean


def test_refused_arguments(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    hashes, strand = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    out = (hashes, None, None, None, n, None)
    # KMU_E_BAD_ARG
    assert raw(ctx, bases, off, *out, s=0)[0] == A.E_BAD_ARG
    assert raw(ctx, bases, off, *out, s=22, s_kmer_type=A.KMER64BIT)[0] == A.E_BAD_ARG          # s > k
    assert raw(ctx, bases, off, *out, t=6)[0] == A.E_BAD_ARG                                       # t > (21 - 11) / 2
    assert raw(ctx, bases, off, *out, s=12, t=5)[0] == A.E_BAD_ARG                                 # t > 9 / 2
    assert raw(ctx, bases, off, *out, s=21, s_kmer_type=A.KMER64BIT, t=1)[0] == A.E_BAD_ARG       # s == k leaves t = 0 only
    assert raw(ctx, bases, off, *out, mem=7)[0] == A.E_BAD_ARG
    hp = A.HashParams(A.KMER64BIT, 21, INV, A.INPUT_ASCII, A.MEM_HOST, 0)
    sp = A.SyncmerParams(A.KMER32BIT, 11, INV, 0)
    P = lambda x: lib._ptr(x)[0]  # noqa: E731
    n_out = C.c_uint64()
    f = ctx.L.kmu_read_syncmers
    assert f(None, C.byref(hp), C.byref(sp), P(bases), P(off), off.size - 1, None, None, None, None, 0, None, C.byref(n_out)) == A.E_BAD_ARG
    assert f(ctx.h, None, C.byref(sp), P(bases), P(off), off.size - 1, None, None, None, None, 0, None, C.byref(n_out)) == A.E_BAD_ARG
    assert f(ctx.h, C.byref(hp), None, P(bases), P(off), off.size - 1, None, None, None, None, 0, None, C.byref(n_out)) == A.E_BAD_ARG
    assert f(ctx.h, C.byref(hp), C.byref(sp), P(bases), P(off), off.size - 1, None, None, None, None, 0, None, None) == A.E_BAD_ARG
    # KMU_E_UNSUPPORTED
    assert raw(ctx, bases, off, *out, input_kind=A.INPUT_PACKED2)[0] == A.E_UNSUPPORTED
    assert raw(ctx, bases, off, hashes, None, None, strand, n, None, fhash=A.FHASH_CANON_NTHASH)[0] == A.E_UNSUPPORTED
    assert raw(ctx, bases, off, None, None, None, None, 0, None, fhash=A.FHASH_CANON_NTHASH)[0] == A.OK
    assert raw(ctx, bases, off, None, None, None, strand, 0, None, s_fhash=A.FHASH_CANON_NTHASH)[0] == A.OK  # fine for the order of the s-mers
    # KMU_E_BAD_ALPHABET: either type
    assert raw(ctx, bases, off, *out, kmer_type=A.KMERAA32BIT)[0] == A.E_BAD_ALPHABET
    assert raw(ctx, bases, off, *out, s=5, s_kmer_type=A.KMERAA32BIT)[0] == A.E_BAD_ALPHABET
    # a (type, size) pair that kmu_kmer_hashes refuses, for k and for s
    assert raw(ctx, bases, off, None, None, None, None, 0, None, kmer_type=A.KMER32BIT)[0] == A.E_BAD_K
    assert raw(ctx, bases, off, None, None, None, None, 0, None, s=15, s_kmer_type=A.KMER32BIT)[0] == A.E_BAD_K
    assert raw(ctx, bases, off, None, None, None, None, 0, None, s=11, s_kmer_type=A.KMER16B32BIT)[0] == A.E_BAD_K
    # no read
    soff = np.full(1, 9, np.uint64)
    assert raw(ctx, np.zeros(16, np.uint8), np.zeros(1, np.uint64), None, None, None, None, 0, soff) == (A.OK, 0) and soff[0] == 0
    same(ctx.read_syncmers(bases, off, BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["s"], BATCH["t"]), want)  # the context still works


# ---- downstream -----------------------------------------------------------------------------------------------------------------------
def test_chains_from_syncmers(ctx, oracle):
    """three reads of 3 kb cut from one random template of 5 kb at 0, 1 000 and 2 000, the middle one reverse-complemented: error-free
    overlaps of 2 kb between neighbours (and 1 kb between the outer two)"""
    k, s, t = 21, 11, 0
    tpl = rand_reads(90, [5000])[0]
    reads = [tpl[0:3000], revcomp(tpl[1000:4000]), tpl[2000:5000]]
    bases, off = oracle.concat(reads)
    q = minimizer.read_syncmers(ctx, bases, off, k, s, t)
    ref = expected_sync(oracle, bases, off, A.KMER64BIT, k, INV, s, t)
    same(q[:5], ref)
    chains = minimizer.chain_hits(ctx, q)
    from_ref = minimizer.chain_hits(ctx, minimizer.Syncmers(*ref, k, s, t, INV))
    assert chains.dtype == np.dtype(A.CHAIN_DTYPE) and chains.tobytes() == from_ref.tobytes()
    # (read_a, read_b, strand, a_start, a_end, b_start, b_end) as planted; read 1 is stored reverse-complemented
    planted = [(0, 1, 1, 1000, 3000, 1000, 3000), (0, 2, 0, 2000, 3000, 0, 1000), (1, 2, 1, 0, 2000, 0, 2000)]
    assert [(c["read_a"], c["read_b"], c["strand"]) for c in chains] == [p[:3] for p in planted]
    for c, p in zip(chains, planted):
        for name, x in zip(("a_start", "a_end", "b_start", "b_end"), p[3:]):
            assert abs(int(c[name]) - x) <= k, (p, name, int(c[name]))
    composed = minimizer.read_chains(ctx, bases, off, k, 10, syncmer=(s, t))
    assert composed.tobytes() == chains.tobytes()
    assert minimizer.read_chains(ctx, bases, off, k, 10).shape == chains.shape  # minimizers find the same three pairs

"""-m gpu: kmu_chain_cigar against `reference_cigar` (tests/test_chain_cigar_abi.py: the contract of include/kmu.h in plain numpy).
Every case compares whole arrays -- records, offsets and runs -- byte for byte, and the records with the PATH bit masked against
Context.chain_align on the same batch.  The chain records are made by hand except in the end-to-end case."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import ALN, HAND_CASES, batch, chain_recs  # noqa: E402
from test_chain_cigar_abi import HAND_CIGARS, reference_cigar, sums, trace_bytes  # noqa: E402
from test_gpu_chain_align import ACGT, band_for, mutate, pair_batch, related  # noqa: E402
from test_gpu_minimizers import rand_reads, revcomp  # noqa: E402

pytestmark = pytest.mark.gpu
MAXD = A.ALIGN_MAX_DIAGS
WALK_BLOCK = 256  # pair-steps the walk has staged at a time, at one pair of diagonals per lane (ALIGN_WALK_ROWS * 8 / C)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def same(got, want, chains, what=""):
    """(aln, ops, op_offsets) equal in every byte"""
    assert got[0].dtype == ALN and got[1].dtype == np.uint32 and got[2].dtype == np.uint64
    assert got[0].shape == want[0].shape and got[2].shape == want[2].shape
    bad = np.nonzero(got[0] != want[0])[0]
    assert bad.size == 0, "%s record %d of %d (chain %s): got %s, want %s" % (what, bad[0], bad.size, chains[bad[0]], got[0][bad[0]], want[0][bad[0]])
    bad = np.nonzero(got[2] != want[2])[0]
    if bad.size:
        c = int(bad[0]) - 1
        raise AssertionError("%s chain %d (%s): runs %s, want %s" % (what, c, chains[c], [hex(v) for v in got[1][int(got[2][c]):int(got[2][c + 1])][:12]],
                                                                       [hex(v) for v in want[1][int(want[2][c]):int(want[2][c + 1])][:12]]))
    bad = np.nonzero(got[1] != want[1])[0]
    if bad.size:
        c = int(np.searchsorted(want[2], bad[0], side="right")) - 1
        raise AssertionError("%s chain %d (%s): run %d is %#x, want %#x" % (what, c, chains[c], bad[0] - int(want[2][c]), got[1][bad[0]], want[1][bad[0]]))


def check(ctx, chains, bases_q, off_q, bases_db=None, off_db=None, band=64, want=None, max_trace_bytes=0):
    """the device's records, offsets and runs equal to the reference's in every byte; the records without PATH equal to chain_align's"""
    if want is None:
        want = reference_cigar(chains, bases_q, off_q, bases_db, off_db, band, max_trace_bytes)
    got = ctx.chain_cigar(chains, bases_q, off_q, bases_db, off_db, band=band, max_trace_bytes=max_trace_bytes)
    same(got, want, chains)
    masked = got[0].copy()
    masked["flags"] &= ~np.uint32(A.ALN_PATH)
    assert masked.tobytes() == ctx.chain_align(chains, bases_q, off_q, bases_db, off_db, band=band).tobytes()
    return got


def permuted(res, perm):
    aln, ops, off = res
    parts = [ops[int(off[c]):int(off[c + 1])] for c in perm]
    new_off = np.zeros(len(perm) + 1, np.uint64)
    new_off[1:] = np.cumsum([p.size for p in parts])
    return aln[perm], np.concatenate(parts) if parts else ops[:0], new_off


# ---- the edges of the band ------------------------------------------------------------------------------------------------------
N_DIAGS = [1, 63, 64, 65, 127, 128, 129, 255, 257, MAXD - 1, MAXD, MAXD + 1]


@pytest.mark.parametrize("n_diags", N_DIAGS)
def test_band_edges(ctx, n_diags):
    """m = 200, n = 200 or 201 (an even n_diags needs an odd |n - m|), both strands; above ALIGN_MAX_DIAGS no runs and no PATH"""
    rng = np.random.default_rng(n_diags)
    delta = n_diags - (MAXD - 1) if n_diags > MAXD else 1 - n_diags % 2
    pairs = [related(rng, 200, 200 + delta), related(rng, 200 + delta, 200)]
    bases, off, chains = pair_batch(pairs, [0, 1])
    aln, ops, op_off = check(ctx, chains, bases, off, band=band_for(n_diags, delta))
    assert (aln["n_diags"] == n_diags).all()
    if n_diags > MAXD:
        assert aln.tolist() == [(0xFFFFFFFF, 0, n_diags, 0)] * 2 and ops.size == 0 and op_off.tolist() == [0, 0, 0]
    else:
        assert (aln["flags"] & A.ALN_PATH).all() and ops.size >= 2


@pytest.mark.parametrize("n_diags", [n for n in N_DIAGS if n >= 63])
def test_band_edges_asymmetric(ctx, n_diags):
    """lo and hi asymmetric: n - m = +-37 where n_diags - 38 is even, +-36 where it is odd"""
    rng = np.random.default_rng(1000 + n_diags)
    delta = 37 if (n_diags - 38) % 2 == 0 else 36
    pairs = [related(rng, 200, 200 + delta), related(rng, 200 + delta, 200), related(rng, 200, 200 + delta), related(rng, 200 + delta, 200)]
    bases, off, chains = pair_batch(pairs, [0, 0, 1, 1])
    aln = check(ctx, chains, bases, off, band=band_for(n_diags, delta))[0]
    assert (aln["n_diags"] == n_diags).all() and ((aln["flags"] & A.ALN_PATH) != 0).all() == (n_diags <= MAXD)


# ---- the edges of the segment lengths -------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, WALK_BLOCK - 2, WALK_BLOCK - 1, WALK_BLOCK, 511, 512, 513, 1025]


@pytest.fixture(scope="module")
def length_batch():
    """read 0: random; read 1: read 0 with 3 % edits; read 2: the reverse complement of read 1.  The chains take the first m bases of
    read 0 against the first n of read 1 -- on strand 1 the last n of read 2, whose reverse complement they are.  m = n = WALK_BLOCK
    - 2, - 1 and + 0 at an even band are WALK_BLOCK - 1, + 0 and + 1 pair-steps"""
    rng = np.random.default_rng(78)
    top = max(LENGTHS)
    r0 = rng.choice(ACGT, top + 60).astype(np.uint8)
    r1 = mutate(rng, r0, 0.03)[0]
    assert r1.size >= top
    reads = [bytes(r0), bytes(r1), revcomp(bytes(r1))]
    off = np.zeros(4, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    rows = []
    for im, m in enumerate(LENGTHS):
        for jn, n in enumerate(LENGTHS):
            s = (im + jn) & 1
            rows.append((0, 2, 1, 0, m, r1.size - n, r1.size) if s else (0, 1, 0, 0, m, 0, n))
            rows.append((0, 1, 0, 0, m, 0, n) if s else (0, 2, 1, 0, m, r1.size - n, r1.size))
    return np.frombuffer(b"".join(reads), np.uint8).copy(), off, chain_recs(rows)


@pytest.mark.parametrize("band,part", [(0, 0), (3, 1), (17, 0)])
def test_segment_length_edges(ctx, length_batch, band, part):
    """every pair of lengths on alternating strands"""
    bases, off, chains = length_batch
    aln = check(ctx, np.ascontiguousarray(chains[part::2]), bases, off, band=band)[0]
    path = (aln["flags"] & A.ALN_PATH) != 0
    assert path.any() and not path.all()  # |n - m| of the long against the short is beyond the band


def test_segment_placement(ctx):
    """the rows of test_gpu_chain_align.test_segment_placement: segments at the first base of the first read, at the last base of
    the last read, and inside reads whose offsets are multiples of neither 4 nor 16"""
    rng = np.random.default_rng(3)
    g = rng.choice(ACGT, 400).astype(np.uint8)
    h = mutate(rng, g, 0.04)[0]
    lens = [37, 101, 250, 333]
    reads = [bytes(g[:37]), bytes(h[20:121]), revcomp(bytes(h[100:350])), bytes(g[60:393])]
    bases, off = np.frombuffer(b"".join(reads), np.uint8).copy(), np.zeros(5, np.uint64)
    off[1:] = np.cumsum(lens)
    rows = [(0, 1, 0, 0, 37, 0, 30), (0, 3, 0, 0, 37, 0, 5), (3, 3, 0, 300, 333, 290, 333), (1, 3, 0, 45, 101, 5, 61),
            (3, 1, 0, 5, 61, 45, 101), (3, 2, 1, 40, 290, 0, 250), (3, 2, 1, 141, 173, 118, 149), (1, 2, 1, 80, 101, 229, 250),
            (3, 3, 1, 333, 333, 333, 333), (0, 0, 0, 0, 0, 0, 0), (3, 0, 1, 332, 333, 0, 1)]
    for band in (0, 4, 40):
        aln, ops, op_off = check(ctx, chain_recs(rows), bases, off, band=band)
    assert aln[7].tolist() == (0, 21, 81, 7) and ops[int(op_off[7]):int(op_off[8])].tolist() == [21 << 4 | 7]
    assert aln[8].tolist() == (0, 0, 81, 7) and op_off[8] == op_off[9] == op_off[10]  # m = n = 0: PATH and no runs


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def test_ties_by_hand(ctx):
    for a, b, band, strand, cigar in HAND_CIGARS:
        bases, off = batch([a, b, "ACGTN"])  # (no segment may be an empty array's address)
        chains = chain_recs([(0, 1, strand, 0, len(a), 0, len(b))])
        got = check(ctx, chains, bases, off, band=band)
        assert minimizer.cigar_strings(got[1], got[2]) == [cigar], (a, b, band, strand)
    for a, b, band, strand, edit, matches in HAND_CASES:
        bases, off = batch([a, b, "ACGTN"])
        got = check(ctx, chain_recs([(0, 1, strand, 0, len(a), 0, len(b))]), bases, off, band=band)
        s = sums(got[1])
        assert (s["X"] + s["I"] + s["D"], s["="]) == (edit, matches)


def test_two_letter_alphabet(ctx):
    """200 random pairs over {A, C} at bands 0 .. 10: nearly every cell ties with a neighbour, and a wrong priority shows"""
    rng = np.random.default_rng(8)
    ac = ACGT[:2]
    for band in range(11):
        pairs = []
        for rep in range(200 // 11 + 1):
            m, n = int(rng.integers(20, 121)), int(rng.integers(20, 121))
            pairs.append(related(rng, m, n, 0.1, ac) if rep % 2 else (rng.choice(ac, m).astype(np.uint8), rng.choice(ac, n).astype(np.uint8)))
        bases, off, chains = pair_batch(pairs, [int(rng.integers(0, 2)) for _ in pairs])
        check(ctx, chains, bases, off, band=band)


# ---- work distribution and purity -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_short():
    """5 000 chains of 5 .. 40 bases inside 64 reads: more chains than one pass of the grid takes"""
    rng = np.random.default_rng(21)
    g = rng.choice(ACGT, 3000).astype(np.uint8)
    reads = []
    for i in range(64):
        s = int(rng.integers(0, 2000))
        r = bytes(mutate(rng, g[s:s + 300 + i], 0.05)[0])
        reads.append(revcomp(r) if i & 1 else r)
    off = np.zeros(65, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    rows = []
    for c in range(5000):
        ra, rb = int(rng.integers(0, 64)), int(rng.integers(0, 64))
        m, n = int(rng.integers(5, 41)), int(rng.integers(5, 41))
        a0, b0 = int(rng.integers(0, len(reads[ra]) - m + 1)), int(rng.integers(0, len(reads[rb]) - n + 1))
        rows.append((ra, rb, c & 1, a0, a0 + m, b0, b0 + n))
    bases, chains = np.frombuffer(b"".join(reads), np.uint8).copy(), chain_recs(rows)
    return bases, off, chains, reference_cigar(chains, bases, off, band=3)


def test_many_short_chains(ctx, many_short):
    bases, off, chains, want = many_short
    got = check(ctx, chains, bases, off, band=3, want=want)
    again = ctx.chain_cigar(chains, bases, off, band=3)  # two calls on one context: identical bytes
    assert all(x.tobytes() == y.tobytes() for x, y in zip(again, got))
    perm = np.random.default_rng(4).permutation(chains.shape[0])
    check(ctx, np.ascontiguousarray(chains[perm]), bases, off, band=3, want=permuted(want, perm))


def test_mixed_routes_in_one_call(ctx):
    """band 20: n_diags = 41 + |n - m| -- chains for 128, 256, 512 and 1024 diagonals and chains that are skipped, interleaved"""
    rng = np.random.default_rng(31)
    pairs, strands = [], []
    for rep in range(4):
        for delta in (0, 150, 400, 900, 1000, -1000, -900, -400, -150, 86, 87, 88, 214, 215, 216, 470, 471, 472, 983, 984):
            m = int(rng.integers(30, 90))
            pairs.append(related(rng, m, m + delta) if delta >= 0 else related(rng, m - delta, m))
            strands.append(len(pairs) & 1)
    bases, off, chains = pair_batch(pairs, strands)
    got = check(ctx, chains, bases, off, band=20)
    assert {41, 127, 128, 129, 191, 255, 256, 257, 441, 511, 512, 513, 941, 1024, 1025, 1041} <= set(got[0]["n_diags"].tolist())
    assert ((got[0]["flags"] & A.ALN_PATH) != 0).tolist() == (got[0]["n_diags"] <= MAXD).tolist()
    perm = np.random.default_rng(5).permutation(chains.shape[0])
    same(ctx.chain_cigar(np.ascontiguousarray(chains[perm]), bases, off, band=20), permuted(got, perm), chains[perm])


# ---- the trace budget -------------------------------------------------------------------------------------------------------------
def test_trace_budget(ctx):
    """40 chains of 100 .. 1 100 bases at the default budget, at a budget that forces at least 4 batches (k_cigar_sweep runs once per
    batch) and at one byte below the largest chain's own trace: the runs of the chains with PATH do not depend on the budget, and the
    oversized chain keeps DONE, edit and matches and has no PATH and no runs.  Context exposes nothing about the size of its
    workspace, so that the call stays within the budget is not asserted here; the batches are cut by the bytes of
    test_chain_cigar_abi.trace_bytes, which this test pins through the oversized chain."""
    rng = np.random.default_rng(41)
    lens = [1100] + [int(v) for v in rng.integers(100, 1000, 39)]
    order = rng.permutation(40)
    pairs = [related(rng, lens[i], lens[i] + int(rng.integers(-20, 21))) for i in order]
    bases, off, chains = pair_batch(pairs, [i & 1 for i in range(40)])
    band = 30
    sizes = [trace_bytes(int(c["a_end"]), int(c["b_end"]), band) for c in chains]
    big = int(np.argmax(sizes))
    assert sorted(sizes)[-1] > sorted(sizes)[-2] and sum(sizes) // 5 >= max(sizes)
    full = check(ctx, chains, bases, off, band=band)
    assert (full[0]["flags"] & A.ALN_PATH).all()
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        cut = ctx.chain_cigar(chains, bases, off, band=band, max_trace_bytes=sum(sizes) // 5)
        n_batches = ctx.profile_get()["k_cigar_sweep"][0]
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    assert n_batches >= 4
    same(cut, full, chains, "budget of a fifth:")
    tight = check(ctx, chains, bases, off, band=band, max_trace_bytes=max(sizes) - 1)
    assert int(tight[0][big]["flags"]) == int(full[0][big]["flags"]) & ~A.ALN_PATH and tight[0][big]["flags"] & A.ALN_DONE
    assert (tight[0][big]["edit"], tight[0][big]["matches"]) == (full[0][big]["edit"], full[0][big]["matches"])
    assert tight[2][big] == tight[2][big + 1]
    keep = np.array([c for c in range(40) if c != big])
    same(permuted(tight, keep), permuted(full, keep), chains[keep], "budget below the largest chain:")
    same(ctx.chain_cigar(chains, bases, off, band=band, max_trace_bytes=max(sizes)), full, chains, "budget of exactly the largest chain:")


# ---- call forms -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(55)
    pairs = [related(rng, int(rng.integers(10, 300)), int(rng.integers(10, 300))) for _ in range(24)]
    bases, off, chains = pair_batch(pairs, [i & 1 for i in range(24)])
    return bases, off, chains, reference_cigar(chains, bases, off, band=30)


def raw(ctx, chains, n, bases_q, off_q, nq, bases_db, off_db, ndb, p, aln, op_off, ops, cap, total, mem=A.MEM_HOST):
    L = lib.load()
    return L.kmu_chain_cigar(ctx.h, lib._ptr(chains)[0], n, lib._ptr(bases_q)[0], lib._ptr(off_q)[0], nq, lib._ptr(bases_db)[0],
                             lib._ptr(off_db)[0], ndb, None if p is None else C.byref(p), mem, lib._ptr(aln)[0], lib._ptr(op_off)[0],
                             lib._ptr(ops)[0], cap, None if total is None else C.byref(total))


def test_count_then_write_one_call_and_capacity(ctx, small):
    bases, off, chains, want = small
    n, n_reads, p = chains.shape[0], off.shape[0] - 1, A.CigarParams(30, 0, 0)
    aln, op_off, total = np.zeros(n, ALN), np.zeros(n + 1, np.uint64), C.c_uint64(0)
    # count only: the records and the offsets are written all the same
    assert raw(ctx, chains, n, bases, off, n_reads, bases, off, n_reads, p, aln, op_off, None, 0, total) == A.OK
    assert total.value == want[1].size and aln.tobytes() == want[0].tobytes() and op_off.tobytes() == want[2].tobytes()
    # one short: refused with the total set, and nothing behind cap is written
    ops = np.full(total.value + 3, 0xABABABAB, np.uint32)
    short = C.c_uint64(0)
    assert raw(ctx, chains, n, bases, off, n_reads, bases, off, n_reads, p, aln, op_off, ops, total.value - 1, short) == A.E_BAD_ARG
    assert short.value == total.value and (ops[total.value - 1:] == 0xABABABAB).all()
    assert raw(ctx, chains, n, bases, off, n_reads, bases, off, n_reads, p, aln, op_off, ops, total.value, short) == A.OK
    assert ops[:total.value].tobytes() == want[1].tobytes() and (ops[total.value:] == 0xABABABAB).all()
    # the one-call form: sized by the records of chain_align
    plain = ctx.chain_align(chains, bases, off, band=30)
    same(ctx.chain_cigar(chains, bases, off, band=30, aln=plain), want, chains, "aln=:")
    assert (np.diff(want[2].astype(np.int64)) <= 2 * plain["edit"].astype(np.int64) + 1).all()


def test_device_tensors_and_self_join(ctx, small):
    import torch
    bases, off, chains, want = small
    got = check(ctx, chains, bases, off, band=30, want=want)
    same(check(ctx, chains, bases, off, bases.copy(), off.copy(), band=30, want=want), got, chains)  # a db batch of its own
    d_chains = torch.from_numpy(chains.view(np.int32).reshape(-1, 10)).cuda()
    d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    d_plain = ctx.chain_align(d_chains, d_bases, d_off, band=30)
    for args, kw in (((d_bases, d_off), {}), ((d_bases, off), {}), ((d_bases, d_off, d_bases.clone(), d_off.clone()), {}),
                     ((d_bases, d_off), {"aln": d_plain}), ((d_bases, d_off), {"max_trace_bytes": 4096})):
        d_aln, d_ops, d_opoff = ctx.chain_cigar(d_chains, *args, band=30, **kw)
        assert d_aln.is_cuda and d_aln.dtype == torch.int32 and tuple(d_aln.shape) == (24, 4)
        assert d_ops.is_cuda and d_ops.dtype == torch.int32 and d_opoff.is_cuda and d_opoff.dtype == torch.int64 and tuple(d_opoff.shape) == (25,)
        if "max_trace_bytes" in kw:
            want_d = reference_cigar(chains, bases, off, band=30, max_trace_bytes=4096)
            assert 0 < ((want_d[0]["flags"] & A.ALN_PATH) != 0).sum() < 24
        else:
            want_d = want
        assert d_aln.cpu().numpy().tobytes() == want_d[0].tobytes() and d_opoff.cpu().numpy().tobytes() == want_d[2].tobytes()
        assert d_ops.cpu().numpy().tobytes() == want_d[1].tobytes()
    # a db batch that differs from q: the b side of every chain moves to a batch of half the reads
    db_reads = [bytes(bases[int(off[2 * i + 1]):int(off[2 * i + 2])]) for i in range(24)]
    db_off = np.zeros(25, np.uint64)
    db_off[1:] = np.cumsum([len(r) for r in db_reads])
    moved = chains.copy()
    moved["read_b"] = np.arange(24)
    same(check(ctx, moved, bases, off, np.frombuffer(b"".join(db_reads), np.uint8).copy(), db_off, band=30), got, moved)
    # no chains
    aln, ops, op_off = ctx.chain_cigar(chains[:0], bases, off, band=30)
    assert aln.shape == (0,) and ops.shape == (0,) and op_off.tolist() == [0]
    d_aln, d_ops, d_opoff = ctx.chain_cigar(d_chains[:0], d_bases, d_off, band=30)
    assert tuple(d_aln.shape) == (0, 4) and tuple(d_ops.shape) == (0,) and d_opoff.cpu().tolist() == [0]


def test_records_the_device_refuses(ctx, small):
    bases, off, chains, want = small
    n_reads = off.shape[0] - 1
    for field, value in (("read_a", n_reads), ("read_b", n_reads), ("read_a", 0xFFFFFFFF), ("strand", 2), ("strand", 0x80000000),
                         ("a_start", int(chains[5]["a_end"]) + 1), ("b_start", 0xFFFFFFFF), ("a_end", int(off[11] - off[10]) + 1),
                         ("b_end", int(off[12] - off[11]) + 1), ("b_end", 0xFFFFFFFF)):
        bad = chains.copy()
        bad[field][5] = value
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_cigar(bad, bases, off, band=30)
        assert e.value.code == A.E_UNSUPPORTED, (field, value)
    check(ctx, chains, bases, off, band=30, want=want)  # the context still works


def test_non_acgt(ctx, small):
    bases, off, chains, _ = small
    sub = chains[:6].copy()  # (the fixture keeps its records: its reference is computed once)
    sub["a_start"][2], sub["a_end"][2] = 3, 8
    sub["b_start"][3], sub["b_end"][3] = 2, 7
    want = reference_cigar(sub, bases, off, band=30)
    for pos in (int(off[4]) + 2, int(off[4]) + 8, int(off[7]) + 1, int(off[7]) + 7, int(off[-1]) - 1):  # right outside segments
        b = bases.copy()
        b[pos] = ord("N")
        check(ctx, sub, b, off, band=30, want=want)
    for pos in (int(off[4]) + 3, int(off[4]) + 7, int(off[7]) + 2, int(off[7]) + 6, 0, int(off[12]) - 1):  # the ends of segments
        b = bases.copy()
        b[pos] = ord("n") if pos & 1 else ord("N")
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_cigar(sub, b, off, band=30)
        assert e.value.code == A.E_NON_ACGT, pos
    # a chain that is skipped does not look at its bases
    b = bases.copy()
    b[int(off[4]) + 3] = ord("N")
    sub["a_end"][2] = 3
    sub["b_end"][3] = 2
    sub["a_end"][0] = 9
    sub["b_end"][0] = 9 + 4  # n_diags = 4 + 2 * 511 + 1
    b[int(off[0]) + 4] = ord("N")
    got = check(ctx, sub, b, off, band=511, want=reference_cigar(sub, bases, off, band=511))
    assert got[0][0].tolist() == (0xFFFFFFFF, 0, MAXD + 3, 0)
    check(ctx, sub, bases, off, band=30)


def test_argument_errors_launch_nothing(ctx, small):
    bases, off, chains, want = small
    n_reads = off.shape[0] - 1
    aln, op_off, ops, total = np.zeros(24, ALN), np.zeros(25, np.uint64), np.zeros(want[1].size, np.uint32), C.c_uint64(0)
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        bad, p = A.E_BAD_ARG, A.CigarParams(30, 0, 0)
        good = (chains, 24, bases, off, n_reads, bases, off, n_reads, p, aln, op_off, ops, ops.size, total)
        for at in (0, 2, 3, 5, 6, 8, 9, 10, 13):  # chains, bases, offsets of either side, p, aln, op_offsets, n_ops
            args = list(good)
            args[at] = None
            assert raw(ctx, *args) == bad, at
        L = lib.load()
        assert L.kmu_chain_cigar(None, lib._ptr(chains)[0], 24, lib._ptr(bases)[0], lib._ptr(off)[0], n_reads, lib._ptr(bases)[0],
                                 lib._ptr(off)[0], n_reads, C.byref(p), A.MEM_HOST, lib._ptr(aln)[0], lib._ptr(op_off)[0],
                                 lib._ptr(ops)[0], ops.size, C.byref(total)) == bad
        for params in (A.CigarParams(30, 1, 0), A.CigarParams(30, 0x80000000, 0), A.CigarParams(MAXD // 2, 0, 0),
                       A.CigarParams(0xFFFFFFFF, 0, 0), A.CigarParams(0x80000000, 0, 0)):
            args = list(good)
            args[8] = params
            assert raw(ctx, *args) == bad, (params.band, params.flags)
        assert raw(ctx, *good, mem=7) == bad
        for at in (4, 7):  # chains while a side has no reads
            args = list(good)
            args[at] = 0
            assert raw(ctx, *args) == bad, at
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_cigar(chains, bases, off, band=MAXD // 2)
        assert e.value.code == bad
        assert (aln == np.zeros(24, ALN)).all() and not op_off.any() and not ops.any()
        total.value, op_off[0] = 5, 9
        args = list(good)
        args[1] = 0  # no chains
        assert raw(ctx, *args) == A.OK and total.value == 0 and op_off[0] == 0
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        assert raw(ctx, *good) == A.OK and total.value == want[1].size  # the context still works
        assert aln.tobytes() == want[0].tobytes() and op_off.tobytes() == want[2].tobytes() and ops.tobytes() == want[1].tobytes()
        assert {"k_cigar_plan", "k_cigar_sweep", "k_cigar_walk", "k_cigar_copy"} <= set(ctx.profile_get())
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
CG = re.compile(r"(\d+)([=XID])")


@pytest.mark.parametrize("opposite", [False, True], ids=["same_strand", "opposite_strand"])
def test_two_reads_of_one_sequence(ctx, opposite):
    """two reads that share genome[1000:2000); read b carries planted edits at about 3 % inside the shared part.  The cg:Z: string
    of the PAF line, replayed over the PAF coordinates -- for strand 1 over the target's forward strand, that is against the reverse
    complement of the query segment -- reproduces columns 10 and 11"""
    k, w, s, e = 15, 10, 1000, 2000
    genome = np.frombuffer(rand_reads(2024, [3000])[0], np.uint8)
    shared, _ = mutate(np.random.default_rng(9), genome[s:e], 0.03)
    read_a, read_b = bytes(genome[0:e]), bytes(shared) + bytes(genome[e:3000])
    reads = [read_a, revcomp(read_b) if opposite else read_b]
    bases = np.frombuffer(b"".join(reads), np.uint8).copy()
    off = np.array([0, len(reads[0]), len(reads[0]) + len(reads[1])], np.uint64)
    chains, aln, ops, op_off = minimizer.read_cigars(ctx, bases, off, k, w, band=32)
    want_chains, want_aln = minimizer.read_alignments(ctx, bases, off, k, w, band=32)
    assert chains.shape == (1,) and chains.tobytes() == want_chains.tobytes() and chains[0]["strand"] == int(opposite)
    same((aln, ops, op_off), reference_cigar(chains, bases, off, band=32), chains)
    assert aln[0]["flags"] == A.ALN_DONE | A.ALN_EXACT | A.ALN_PATH and aln[0]["edit"] == want_aln[0]["edit"] > 0
    line = minimizer.paf_lines(chains, aln, ["a", "b"], off, cigar=(ops, op_off))[0].split("\t")
    assert line[:15] == minimizer.paf_lines(chains, aln, ["a", "b"], off)[0].split("\t") and line[15].startswith("cg:Z:") and len(line) == 16
    q = reads[0][int(line[2]):int(line[3])]
    t = reads[1][int(line[7]):int(line[8])]
    if line[4] == "-":
        q = revcomp(q)
    i = j = matches = block = 0
    for n, op in ((int(n), op) for n, op in CG.findall(line[15][5:])):
        if op in "=X":
            assert all((q[i + x] == t[j + x]) == (op == "=") for x in range(n))
            matches += n if op == "=" else 0
        i, j, block = i + (n if op != "D" else 0), j + (n if op != "I" else 0), block + n
    assert (i, j) == (len(q), len(t)) and "".join("%s%s" % r for r in CG.findall(line[15][5:])) == line[15][5:]
    assert [str(matches), str(block)] == line[9:11] and line[12] == "NM:i:%d" % (block - matches)
    # the same on resident arrays
    import torch
    d = minimizer.read_cigars(ctx, torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), k, w, band=32)
    assert all(x.is_cuda for x in d)
    assert [x.cpu().numpy().tobytes() for x in d] == [chains.tobytes(), aln.tobytes(), ops.tobytes(), op_off.tobytes()]

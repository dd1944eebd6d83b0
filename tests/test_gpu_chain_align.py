"""-m gpu: kmu_chain_align against `reference_align` (tests/test_chain_align_abi.py: the contract of include/kmu.h in plain numpy).
Every case compares whole record arrays byte for byte; the chain records are made by hand except in the end-to-end case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chain_align_abi import (ALN, HAND_CASES, batch, chain_recs, full_matrix, narrow_band_case, reference_align,  # noqa: E402
                                  revcomp as revcomp_str)
from test_chains_abi import reference_chains  # noqa: E402
from test_gpu_minimizers import expected, rand_reads, reference_hits, revcomp  # noqa: E402

pytestmark = pytest.mark.gpu
MAXD, CHUNK = A.ALIGN_MAX_DIAGS, A.ALIGN_CHUNK
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def check(ctx, chains, bases_q, off_q, bases_db=None, off_db=None, band=64, want=None):
    """the device's records, equal to the reference's in every byte"""
    if want is None:
        want = reference_align(chains, bases_q, off_q, bases_db, off_db, band)
    got = ctx.chain_align(chains, bases_q, off_q, bases_db, off_db, band=band)
    assert got.dtype == ALN and got.shape == want.shape
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "record %d of %d (chain %s, band %d): got %s, want %s" % (bad[0], bad.size, chains[bad[0]], band, got[bad[0]], want[bad[0]])
    return got


def mutate(rng, s, rate, alpha=ACGT):
    """s (uint8 array) with substitutions, insertions and deletions at `rate`; returns (copy, number of edits)"""
    out, edits = [], 0
    for c in s.tolist():
        r = rng.random()
        if r < rate / 3:
            out.append(int(rng.choice(alpha[alpha != c])))
        elif r < 2 * rate / 3:
            out += [int(rng.choice(alpha)), c]
        elif r < rate:
            pass
        else:
            out.append(c)
            continue
        edits += 1
    return np.array(out, np.uint8), edits


def related(rng, m, n, rate=0.05, alpha=ACGT):
    """a random string of m letters and a copy of it with edits at `rate`, cut or filled up to n letters"""
    a = rng.choice(alpha, m).astype(np.uint8)
    b = mutate(rng, a, rate, alpha)[0][:n]
    return a, np.concatenate([b, rng.choice(alpha, n - b.size).astype(np.uint8)])


def pair_batch(pairs, strands=None):
    """every (a, b) of pairs as two reads of one batch (a: read 2 i, b: read 2 i + 1, stored reverse-complemented where its strand is
    1) and the chain records that take them whole"""
    strands = [0] * len(pairs) if strands is None else strands
    reads, rows = [], []
    for i, ((a, b), s) in enumerate(zip(pairs, strands)):
        a, b = bytes(a), bytes(b)
        reads += [a, revcomp(b) if s else b]
        rows.append((2 * i, 2 * i + 1, s, 0, len(a), 0, len(b)))
    off = np.zeros(len(reads) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in reads])
    return np.frombuffer(b"".join(reads) + b"", np.uint8).copy(), off, chain_recs(rows)


# ---- the edges of the band ------------------------------------------------------------------------------------------------------
def band_for(n_diags, delta):
    assert (n_diags - abs(delta) - 1) % 2 == 0 and n_diags - abs(delta) - 1 >= 0
    return (n_diags - abs(delta) - 1) // 2


N_DIAGS = [1, 63, 64, 65, 127, 128, 129, 255, 257, MAXD - 1, MAXD, MAXD + 1, MAXD + 2]


@pytest.mark.parametrize("n_diags", N_DIAGS)
def test_band_edges(ctx, n_diags):
    """m = 200, n = 200 or 201 (an even n_diags needs an odd |n - m|); above ALIGN_MAX_DIAGS the largest band the call takes, 511,
    and |n - m| = 2 and 3"""
    rng = np.random.default_rng(n_diags)
    delta = n_diags - (MAXD - 1) if n_diags > MAXD else 1 - n_diags % 2
    pairs = [related(rng, 200, 200 + delta), related(rng, 200 + delta, 200)]
    bases, off, chains = pair_batch(pairs, [0, 1])
    got = check(ctx, chains, bases, off, band=band_for(n_diags, delta))
    assert (got["n_diags"] == n_diags).all()
    if n_diags > MAXD:
        assert got.tolist() == [(0xFFFFFFFF, 0, n_diags, 0)] * 2
    else:
        assert (got["flags"] & A.ALN_DONE).all() and (n_diags < 63 or (got["edit"] < 60).all())


@pytest.mark.parametrize("n_diags", [n for n in N_DIAGS if n >= 63])
def test_band_edges_asymmetric(ctx, n_diags):
    """lo and hi asymmetric: n - m = +-37 where n_diags - 38 is even, +-36 where it is odd (2 band = n_diags - |n - m| - 1)"""
    rng = np.random.default_rng(1000 + n_diags)
    delta = 37 if (n_diags - 38) % 2 == 0 else 36
    pairs = [related(rng, 200, 200 + delta), related(rng, 200 + delta, 200), related(rng, 200, 200 + delta), related(rng, 200 + delta, 200)]
    bases, off, chains = pair_batch(pairs, [0, 0, 1, 1])
    got = check(ctx, chains, bases, off, band=band_for(n_diags, delta))
    assert (got["n_diags"] == n_diags).all() and ((got["flags"] & A.ALN_DONE) != 0).all() == (n_diags <= MAXD)


# ---- the edges of the segment lengths -------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 31, 32, 33, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


@pytest.fixture(scope="module")
def length_batch():
    """read 0: random; read 1: read 0 with 3 % edits; read 2: the reverse complement of read 1.  The chains take the first m bases of
    read 0 against the first n of read 1 -- on strand 1 the last n of read 2, whose reverse complement they are"""
    rng = np.random.default_rng(77)
    top = 2 * CHUNK + 1
    r0 = rng.choice(ACGT, top + 40).astype(np.uint8)
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


@pytest.mark.parametrize("band,part", [(0, 0), (3, 1), (17, 0), (17, 1)])
def test_segment_length_edges(ctx, length_batch, band, part):
    """every pair of lengths: on both strands at band 17, on alternating strands at bands 0 and 3"""
    bases, off, chains = length_batch
    got = check(ctx, np.ascontiguousarray(chains[part::2]), bases, off, band=band)
    done = (got["flags"] & A.ALN_DONE) != 0
    assert done.any() and not done.all()  # |n - m| of the long against the short is beyond the band


def test_segment_placement(ctx):
    """segments at the first base of the first read, at the last base of the last read, and inside reads whose offsets are
    multiples of neither 4 nor 16"""
    rng = np.random.default_rng(3)
    g = rng.choice(ACGT, 400).astype(np.uint8)
    h = mutate(rng, g, 0.04)[0]
    lens = [37, 101, 250, 333]
    reads = [bytes(g[:37]), bytes(h[20:121]), revcomp(bytes(h[100:350])), bytes(g[60:393])]
    bases, off = np.frombuffer(b"".join(reads), np.uint8).copy(), np.zeros(5, np.uint64)
    off[1:] = np.cumsum(lens)
    assert [int(o) % 4 for o in off[1:4]] == [1, 2, 0] and int(off[2]) % 16 and int(off[3]) % 16
    rows = [(0, 1, 0, 0, 37, 0, 30),        # g[0:37] against h[20:50]: the first base of the first read
            (0, 3, 0, 0, 37, 0, 5),
            (3, 3, 0, 300, 333, 290, 333),  # the last base of the last read, on both sides
            (1, 3, 0, 45, 101, 5, 61),      # h[65:121] against g[65:121]
            (3, 1, 0, 5, 61, 45, 101),
            (3, 2, 1, 40, 290, 0, 250),     # g[100:350] against the reverse complement of read 2 = h[100:350]
            (3, 2, 1, 141, 173, 118, 149),  # inside both
            (1, 2, 1, 80, 101, 229, 250),   # h[100:121] twice
            (3, 3, 1, 333, 333, 333, 333), (0, 0, 0, 0, 0, 0, 0), (3, 0, 1, 332, 333, 0, 1)]
    for band in (0, 4, 40):
        got = check(ctx, chain_recs(rows), bases, off, band=band)
    assert got[7].tolist() == (0, 21, 81, 3) and got[8].tolist() == (0, 0, 81, 3)


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def test_ties_by_hand(ctx):
    for a, b, band, strand, edit, matches in HAND_CASES:
        bases, off = batch([a, b, "ACGTN"])  # (no segment may be an empty array's address)
        got = check(ctx, chain_recs([(0, 1, strand, 0, len(a), 0, len(b))]), bases, off, band=band)
        assert (int(got[0]["edit"]), int(got[0]["matches"])) == (edit, matches)


def test_two_letter_alphabet(ctx):
    """200 random pairs over {A, C}: nearly every cell ties with a neighbour"""
    rng = np.random.default_rng(8)
    ac = ACGT[:2]
    for band in range(11):
        pairs = []
        for rep in range(200 // 11 + 1):
            m, n = int(rng.integers(20, 121)), int(rng.integers(20, 121))
            pairs.append(related(rng, m, n, 0.1, ac) if rep % 2 else (rng.choice(ac, m).astype(np.uint8), rng.choice(ac, n).astype(np.uint8)))
        bases, off, chains = pair_batch(pairs, [int(rng.integers(0, 2)) for _ in pairs])
        check(ctx, chains, bases, off, band=band)


def test_exact_flag(ctx):
    a, b = narrow_band_case()
    bases, off = batch([a, b])
    chains = chain_recs([(0, 1, 0, 0, len(a), 0, len(b))])
    narrow, wide = check(ctx, chains, bases, off, band=2)[0], check(ctx, chains, bases, off, band=16)[0]
    assert narrow["flags"] == A.ALN_DONE and wide["flags"] == A.ALN_DONE | A.ALN_EXACT
    assert (int(wide["edit"]), int(wide["matches"])) == full_matrix(a, b) and narrow["edit"] > wide["edit"]


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
    return bases, off, chains, reference_align(chains, bases, off, band=3)


def test_many_short_chains(ctx, many_short):
    bases, off, chains, want = many_short
    got = check(ctx, chains, bases, off, band=3, want=want)
    again = ctx.chain_align(chains, bases, off, band=3)  # two calls on one context: identical bytes
    assert again.tobytes() == got.tobytes()
    perm = np.random.default_rng(4).permutation(chains.shape[0])
    check(ctx, np.ascontiguousarray(chains[perm]), bases, off, band=3, want=want[perm])


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
    nd = set(got["n_diags"].tolist())
    assert {41, 127, 128, 129, 191, 255, 256, 257, 441, 511, 512, 513, 941, 1024, 1025, 1041} <= nd
    assert ((got["flags"] & A.ALN_DONE) != 0).tolist() == (got["n_diags"] <= MAXD).tolist()
    perm = np.random.default_rng(5).permutation(chains.shape[0])
    assert ctx.chain_align(np.ascontiguousarray(chains[perm]), bases, off, band=20).tobytes() == got[perm].tobytes()


# ---- call forms -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(55)
    pairs = [related(rng, int(rng.integers(10, 300)), int(rng.integers(10, 300))) for _ in range(24)]
    return pair_batch(pairs, [i & 1 for i in range(24)])


def test_device_tensors_and_self_join(ctx, small):
    import torch
    bases, off, chains = small
    got = check(ctx, chains, bases, off, band=30)
    assert check(ctx, chains, bases, off, bases.copy(), off.copy(), band=30).tobytes() == got.tobytes()  # a db batch of its own
    d_chains = torch.from_numpy(chains.view(np.int32).reshape(-1, 10)).cuda()
    d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    for args in ((d_bases, d_off), (d_bases, off), (d_bases, d_off, d_bases.clone(), d_off.clone())):
        d = ctx.chain_align(d_chains, *args, band=30)
        assert d.is_cuda and d.dtype == torch.int32 and tuple(d.shape) == (24, 4)
        assert d.cpu().numpy().tobytes() == got.tobytes()
    # a db batch that differs from q: the b side of every chain moves to a batch of half the reads
    db_reads = [bytes(bases[int(off[2 * i + 1]):int(off[2 * i + 2])]) for i in range(24)]
    db_off = np.zeros(25, np.uint64)
    db_off[1:] = np.cumsum([len(r) for r in db_reads])
    moved = chains.copy()
    moved["read_b"] = np.arange(24)
    assert check(ctx, moved, bases, off, np.frombuffer(b"".join(db_reads), np.uint8).copy(), db_off, band=30).tobytes() == got.tobytes()
    # no chains
    assert ctx.chain_align(chains[:0], bases, off, band=30).shape == (0,)
    assert tuple(ctx.chain_align(d_chains[:0], d_bases, d_off, band=30).shape) == (0, 4)


def raw(ctx, chains, n, bases_q, off_q, nq, bases_db, off_db, ndb, p, out, mem=A.MEM_HOST):
    L = lib.load()
    rc = L.kmu_chain_align(ctx.h, lib._ptr(chains)[0], n, lib._ptr(bases_q)[0], lib._ptr(off_q)[0], nq, lib._ptr(bases_db)[0],
                           lib._ptr(off_db)[0], ndb, None if p is None else C.byref(p), mem, lib._ptr(out)[0])
    return rc


def test_records_the_device_refuses(ctx, small):
    bases, off, chains = small
    n_reads = off.shape[0] - 1
    len1 = int(off[2] - off[1])
    for field, value in (("read_a", n_reads), ("read_b", n_reads), ("read_a", 0xFFFFFFFF), ("strand", 2), ("strand", 0x80000000),
                         ("a_start", int(chains[5]["a_end"]) + 1), ("b_start", 0xFFFFFFFF), ("a_end", int(off[11] - off[10]) + 1),
                         ("b_end", int(off[12] - off[11]) + 1), ("b_end", 0xFFFFFFFF)):
        bad = chains.copy()
        bad[field][5] = value
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_align(bad, bases, off, band=30)
        assert e.value.code == A.E_UNSUPPORTED, (field, value)
    assert len1 > 0
    check(ctx, chains, bases, off, band=30)  # the context still works


def test_non_acgt(ctx, small):
    bases, off, chains = small
    sub = np.ascontiguousarray(chains[:6])
    sub["a_start"][2], sub["a_end"][2] = 3, 8
    sub["b_start"][3], sub["b_end"][3] = 2, 7
    want = reference_align(sub, bases, off, band=30)
    for pos in (int(off[4]) + 2, int(off[4]) + 8, int(off[7]) + 1, int(off[7]) + 7, int(off[-1]) - 1):  # right outside segments
        b = bases.copy()
        b[pos] = ord("N")
        check(ctx, sub, b, off, band=30, want=want)
    for pos in (int(off[4]) + 3, int(off[4]) + 7, int(off[7]) + 2, int(off[7]) + 6, 0, int(off[12]) - 1):  # the ends of segments
        b = bases.copy()
        b[pos] = ord("n") if pos & 1 else ord("N")
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_align(sub, b, off, band=30)
        assert e.value.code == A.E_NON_ACGT, pos
    # a chain that is skipped does not look at its bases
    b = bases.copy()
    b[int(off[4]) + 3] = ord("N")
    sub["a_end"][2] = 3
    sub["b_end"][3] = 2
    sub["a_end"][0] = 9
    sub["b_end"][0] = 9 + 4  # n_diags = 4 + 2 * 511 + 1
    b[int(off[0]) + 4] = ord("N")
    got = check(ctx, sub, b, off, band=511, want=reference_align(sub, bases, off, band=511))
    assert got[0].tolist() == (0xFFFFFFFF, 0, MAXD + 3, 0)
    check(ctx, sub, bases, off, band=30)


def test_argument_errors_launch_nothing(ctx, small):
    bases, off, chains = small
    n_reads = off.shape[0] - 1
    out = np.zeros(24, ALN)
    ctx.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        bad, p = A.E_BAD_ARG, A.AlignParams(30, 0)
        good = (chains, 24, bases, off, n_reads, bases, off, n_reads, p, out)
        for at in (0, 2, 3, 5, 6, 8, 9):  # chains, bases, offsets of either side, p, out
            args = list(good)
            args[at] = None
            assert raw(ctx, *args) == bad, at
        L = lib.load()
        assert L.kmu_chain_align(None, lib._ptr(chains)[0], 24, lib._ptr(bases)[0], lib._ptr(off)[0], n_reads, lib._ptr(bases)[0],
                                 lib._ptr(off)[0], n_reads, C.byref(p), A.MEM_HOST, lib._ptr(out)[0]) == bad
        for params in (A.AlignParams(30, 1), A.AlignParams(30, 0x80000000), A.AlignParams(MAXD // 2, 0), A.AlignParams(0xFFFFFFFF, 0),
                       A.AlignParams(0x80000000, 0)):
            args = list(good)
            args[8] = params
            assert raw(ctx, *args) == bad, (params.band, params.flags)
        assert raw(ctx, *good, mem=7) == bad
        for at in (4, 7):  # chains while a side has no reads
            args = list(good)
            args[at] = 0
            assert raw(ctx, *args) == bad, at
        with pytest.raises(lib.KmuError) as e:
            ctx.chain_align(chains, bases, off, band=MAXD // 2)
        assert e.value.code == bad
        assert (out == np.zeros(24, ALN)).all()
        assert ctx.chain_align(chains[:0], bases, off, band=30).shape == (0,)
        ctx.synchronize()
        assert ctx.profile_get() == {}, "a refused or empty call launched a kernel"
        check(ctx, chains, bases, off, band=(MAXD - 1) // 2)  # the widest band the call takes; the context still works
        assert "k_chain_align" in ctx.profile_get()
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opposite", [False, True], ids=["same_strand", "opposite_strand"])
def test_two_reads_of_one_sequence(ctx, oracle, opposite):
    """two reads that share genome[1000:2000); read b carries planted edits at about 3 % inside the shared part"""
    k, w, s, e = 15, 10, 1000, 2000
    genome = np.frombuffer(rand_reads(2024, [3000])[0], np.uint8)
    rng = np.random.default_rng(9)
    shared, n_edits = mutate(rng, genome[s:e], 0.03)
    read_a, read_b = bytes(genome[0:e]), bytes(shared) + bytes(genome[e:3000])
    reads = [read_a, revcomp(read_b) if opposite else read_b]
    bases, off = oracle.concat(reads)
    # on the CPU first: the oracle's hashes, the reference minimizers, a dict join and the reference chains give one chain of at
    # least 3 seeds
    hashes, pos, read, strand, moff = expected(oracle, bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
    mm = minimizer.Minimizers(hashes, pos, read, strand, moff, k, w, A.FHASH_CANON_INVHASH)
    hits = sorted(h for h in reference_hits(mm, mm, True, 0) if h[0] == 0)
    index = {(int(rd), int(p)): i for i, (rd, p) in enumerate(zip(read, pos))}
    pairs = np.array([(index[(h[0], h[1])], index[(h[3], h[4])]) for h in hits], np.uint32)
    want_chains = reference_chains(pairs, mm, mm, k, 5000, 500, min_seeds=3, upper=True)
    assert want_chains.shape == (1,) and want_chains[0]["n_seeds"] >= 3 and want_chains[0]["strand"] == int(opposite)

    chains, aln = minimizer.read_alignments(ctx, bases, off, k, w, band=32)
    assert np.array_equal(chains, want_chains) and aln.dtype == ALN and aln.shape == (1,)
    assert aln.tobytes() == reference_align(chains, bases, off, band=32).tobytes()
    r, c = aln[0], chains[0]
    m, n = int(c["a_end"]) - int(c["a_start"]), int(c["b_end"]) - int(c["b_start"])
    assert r["flags"] == A.ALN_DONE | A.ALN_EXACT and r["n_diags"] == abs(n - m) + 65
    assert m > 800 and 0 < r["edit"] <= n_edits  # the segment ends are matching seeds: the planted edits inside are one alignment of it
    assert int(r["matches"]) + int(r["edit"]) >= max(m, n)
    line = minimizer.paf_lines(chains, aln, ["a", "b"], off)[0].split("\t")
    assert line[:2] == ["a", "2000"] and line[4] == "+-"[opposite] and line[9:13] == [str(r["matches"]), str(r["matches"] + r["edit"]), "255", "NM:i:%d" % r["edit"]]
    # the same on resident arrays
    import torch
    d_chains, d_aln = minimizer.read_alignments(ctx, torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), k, w, band=32)
    assert d_aln.is_cuda and d_chains.cpu().numpy().tobytes() == chains.tobytes() and d_aln.cpu().numpy().tobytes() == aln.tobytes()

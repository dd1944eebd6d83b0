"""-m gpu: kmu_read_minimizers against `reference_minimizers` (tests/test_minimizers_abi.py: the rules of include/kmu.h as plain
numpy, checked there against a brute force) over the oracle's kmer_hashes.  The strand reference is "the canonical value differs
from the forward value" at the chosen position.  Every case compares whole arrays exactly."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_minimizers_abi import n_windows, reference_minimizers  # noqa: E402

pytestmark = pytest.mark.gpu
T = A.MINIMIZER_TILE
MAX_W = A.MINIMIZER_MAX_W
CANON = (A.FHASH_CANON_RAW, A.FHASH_CANON_VALUE, A.FHASH_CANON_INVHASH)
NTHASH = (A.FHASH_CANON_NTHASH, A.FHASH_CANON_NTHASH_8B)
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def rand_reads(seed, lens):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(ACGT, size=int(n))) for n in lens]


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def host(x):
    """a numpy view of the bits of a result array (device tensors come back as int64 / int32 / uint8)"""
    if x is None:
        return None
    if type(x).__module__.startswith("torch"):
        x = x.cpu().numpy()
    x = np.ascontiguousarray(x)
    return x.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[x.dtype.itemsize])


def expected(oracle, bases, off, kmer_type, k, fhash, w, h=None):
    """(hashes, pos, read, strand or None, mini_offsets) of the reads bases[off[0] : off[-1]]"""
    off = np.asarray(off, np.uint64)
    sub = np.ascontiguousarray(bases[int(off[0]):max(int(off[-1]), int(off[0]) + 1)])
    off0 = off - off[0]
    if h is None:
        h = oracle.kmer_hashes(sub, off0, kmer_type, k, fhash)
    hashes, pos, read, moff = reference_minimizers(h, off0, k, w)
    strand = None
    if fhash not in NTHASH:
        strand = np.zeros(pos.size, np.uint8)
        if fhash in CANON:
            differs = oracle.kmer_hashes(sub, off0, kmer_type, k, A.FHASH_CANON_VALUE) != oracle.kmer_hashes(sub, off0, kmer_type, k, A.FHASH_VALUE_MASKED)
            strand = differs[off0[read.astype(np.int64)].astype(np.int64) + pos.astype(np.int64)].astype(np.uint8)
    return hashes, pos, read, strand, moff


def same(got, want, what=""):
    names = ("hashes", "pos", "read", "strand", "mini_offsets")
    for name, g, x in zip(names, got, want):
        g = host(g)
        if x is None:
            assert g is None, name
            continue
        assert g.shape == x.shape, "%s %s: %d entries, want %d" % (what, name, g.size, x.size)
        bad = np.nonzero(g != x)[0]
        assert bad.size == 0, "%s %s differs at %s: got %s, want %s" % (what, name, bad[:6].tolist(), g[bad[:6]], x[bad[:6]])


def check(ctx, oracle, reads, kmer_type, k, fhash, w, h=None):
    bases, off = oracle.concat(reads)
    want = expected(oracle, bases, off, kmer_type, k, fhash, w, h)
    got = ctx.read_minimizers(bases, off, kmer_type, k, fhash, w, want=("pos", "read") if fhash in NTHASH else lib.MINIMIZERS_WANT)
    same(got, want, "w = %d" % w)
    return [host(g) for g in got]


# ---- parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fhash", [A.FHASH_CANON_INVHASH, A.FHASH_CANON_VALUE, A.FHASH_VALUE_MASKED, A.FHASH_CANON_NTHASH],
                         ids=["canon_invhash", "canon_value", "value_masked", "canon_nthash"])
@pytest.mark.parametrize("kmer_type,k", [(A.KMER32BIT, 11), (A.KMER16B32BIT, 16), (A.KMER64BIT, 21), (A.KMER64BIT, 31)])
def test_parity(ctx, oracle, kmer_type, k, fhash):
    lens = np.random.default_rng(k).integers(1, 3001, size=40)
    reads = rand_reads(100 + k, lens)
    bases, off = oracle.concat(reads)
    h = oracle.kmer_hashes(bases, off, kmer_type, k, fhash)
    for w in (1, 5, 10, 19):
        got = check(ctx, oracle, reads, kmer_type, k, fhash, w, h)
        if w == 1:  # every k-mer
            want_pos = np.concatenate([np.arange(max(0, int(n) - k + 1)) for n in lens])
            assert np.array_equal(got[1], want_pos)


# ---- window edges ---------------------------------------------------------------------------------------------------------------
def test_window_edges(ctx, oracle):
    k, w = 21, 10
    lens = [0, 1, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w, k + w + 1]
    got = check(ctx, oracle, rand_reads(1, lens), A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
    n = np.diff(got[4].astype(np.int64))
    assert n[:3].tolist() == [0, 0, 0] and (n[3:7] == 1).all() and (n <= [n_windows(x, k, w) for x in lens]).all()


def test_widest_window(ctx, oracle):
    k, w = 21, MAX_W
    lens = [nk + k - 1 for nk in (w - 1, w, w + 1)] + [3 * w + 7]
    got = check(ctx, oracle, rand_reads(2, lens), A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
    assert np.diff(got[4].astype(np.int64))[:2].tolist() == [1, 1]


# ---- tiles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 64, MAX_W])
def test_tile_boundaries(ctx, oracle, w):
    k = 21
    lens = [nwin + w - 1 + k - 1 for nwin in (T - 1, T, T + 1, 2 * T + 1)]
    assert [n_windows(x, k, w) for x in lens] == [T - 1, T, T + 1, 2 * T + 1]
    check(ctx, oracle, rand_reads(3 + w, lens), A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)


@pytest.mark.parametrize("q", [T + 32, 2 * T - 1, 2 * T], ids=["T+w/2", "2T-1", "2T"])
def test_planted_minimum_at_a_tile_boundary(ctx, oracle, q):
    """the k-mer A^k (value 0 under VALUE_MASKED) at position q: windows of two tiles choose it, it comes out once"""
    k, w = 21, 64
    read = bytearray(rand_reads(11, [3 * T])[0])
    read[q - 1:q + k + 1] = b"C" + b"A" * k + b"C"
    got = check(ctx, oracle, [bytes(read)], A.KMER64BIT, k, A.FHASH_VALUE_MASKED, w)
    assert int((got[1] == q).sum()) == 1 and got[0][got[1] == q][0] == 0


@pytest.mark.parametrize("fhash", [A.FHASH_CANON_VALUE, A.FHASH_VALUE_MASKED], ids=["canon_value", "value_masked"])
def test_ties_across_tiles(ctx, oracle, fhash):
    k, w = 21, 19
    got = check(ctx, oracle, [b"A" * 5000], A.KMER64BIT, k, fhash, w)
    assert np.array_equal(got[1], np.arange(n_windows(5000, k, w)))  # every window start, nothing behind
    check(ctx, oracle, [b"ACGT" * 1300, b"AC" * 2600], A.KMER64BIT, k, fhash, w)
    check(ctx, oracle, [b"AC" * 2600, b"A" * 5000], A.KMER64BIT, k, fhash, MAX_W)


def test_many_short_reads(ctx, oracle):
    lens = np.random.default_rng(5).integers(30, 61, size=5000)
    got = check(ctx, oracle, rand_reads(6, lens), A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, 10)
    assert int(got[4][-1]) == got[0].size


def test_more_tiles_than_a_fresh_workspace_holds(oracle):
    """A device call does not know its number of tiles: it counts into the workspace the context has (65 536 tiles in a fresh
    one) and counts again when they did not fit.  66 000 reads of one window each are 66 000 tiles; then a small batch on the
    grown workspace, whose entries behind the last tile must count as nothing."""
    import torch
    k, w = 21, 10
    lens = np.random.default_rng(14).integers(k, k + w, size=66000)
    reads = rand_reads(15, lens)
    bases, off = oracle.concat(reads)
    want = expected(oracle, bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
    assert want[0].size == 66000
    c = lib.Context(0)
    try:
        d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
        same(c.read_minimizers(d_bases, d_off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w), want, "fresh")
        few = expected(oracle, bases, off[:8], A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
        same(c.read_minimizers(d_bases, d_off[:8].clone(), A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w), few, "grown")
    finally:
        c.close()


def test_one_long_read(ctx, oracle):
    got = check(ctx, oracle, rand_reads(7, [300000]), A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, 19)
    assert int(got[1].max()) > 65535 and (np.diff(got[1].astype(np.int64)) > 0).all()


def test_reverse_complement(ctx, oracle):
    k, w = 21, 10
    reads = rand_reads(8, [1500, 77, 3000, 21, 2 * T + 100])
    bases, off = oracle.concat(reads)
    fw = [host(x) for x in ctx.read_minimizers(bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)]
    bases_rc, _ = oracle.concat([revcomp(s) for s in reads])
    rc = [host(x) for x in ctx.read_minimizers(bases_rc, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)]
    assert np.array_equal(fw[4], rc[4])
    for i, s in enumerate(reads):
        b, e = int(fw[4][i]), int(fw[4][i + 1])
        assert np.array_equal(rc[1][b:e][::-1], len(s) - k - fw[1][b:e])  # mirrored positions
        assert np.array_equal(rc[0][b:e][::-1], fw[0][b:e])               # the same hashes
        assert np.array_equal(rc[3][b:e][::-1], 1 - fw[3][b:e])           # k is odd: no k-mer is its own reverse complement


# ---- buffers and calls ------------------------------------------------------------------------------------------------------------
BATCH = dict(kmer_type=A.KMER64BIT, k=21, fhash=A.FHASH_CANON_INVHASH, w=10)


@pytest.fixture(scope="module")
def batch(oracle):
    reads = rand_reads(9, [333, 700, 41, 1200, 515, 90, 0, 20, 2500])
    bases, off = oracle.concat(reads)
    want = expected(oracle, bases, off, BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["w"])
    return bases, off, want


def raw(ctx, bases, off, hashes, pos, read, strand, cap, moff, mem=A.MEM_HOST, w=None, kmer_type=None, fhash=None, input_kind=A.INPUT_ASCII):
    """kmu_read_minimizers through the raw C-ABI: (status, *n_out)"""
    hp = A.HashParams(BATCH["kmer_type"] if kmer_type is None else kmer_type, BATCH["k"], BATCH["fhash"] if fhash is None else fhash, input_kind, mem, 0)
    total = C.c_uint64(0xDEAD)
    P = lambda x: lib._ptr(x)[0]  # noqa: E731
    rc = ctx.L.kmu_read_minimizers(ctx.h, C.byref(hp), P(bases), P(off), len(off) - 1, BATCH["w"] if w is None else w, P(hashes), P(pos),
                                   P(read), P(strand), cap, P(moff), C.byref(total))
    return rc, int(total.value)


def test_batch_that_starts_inside_a_larger_array(ctx, oracle, batch):
    import torch
    bases, off, _ = batch
    first, last = 2, 6
    want = expected(oracle, bases, off[first:last + 1], **BATCH)
    same(ctx.read_minimizers(bases, off[first:last + 1].copy(), BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["w"]), want, "host")
    d_bases = torch.from_numpy(bases).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    same(ctx.read_minimizers(d_bases, d_off[first:last + 1], BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["w"]), want, "device")


def test_device_tensors_give_the_same_bits(ctx, batch):
    import torch
    bases, off, want = batch
    got = ctx.read_minimizers(torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), BATCH["kmer_type"], BATCH["k"],
                              BATCH["fhash"], BATCH["w"])
    assert all(x.is_cuda for x in got)
    assert [x.dtype for x in got] == [torch.int64, torch.int32, torch.int32, torch.uint8, torch.int64]
    same(got, want)


def test_count_only_call_writes_nothing_else(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    pos, read, strand = np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5A5A5A5, np.uint32), np.full(n, 0xA5, np.uint8)
    moff = np.full(off.size, 77, np.uint64)
    assert raw(ctx, bases, off, None, pos, read, strand, n, moff) == (A.OK, n)
    assert (pos == 0xA5A5A5A5).all() and (read == 0xA5A5A5A5).all() and (strand == 0xA5).all()
    assert np.array_equal(moff, want[4])
    assert raw(ctx, bases, off, None, None, None, None, 0, None) == (A.OK, n)


def test_cap_rules(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    hashes = np.zeros(n, np.uint64)
    assert raw(ctx, bases, off, hashes, None, None, None, n - 1, None) == (A.E_BAD_ARG, n)
    # the layout's bound, with no count-only call in front
    cap = int(lib.minimizer_layout(off, BATCH["k"], BATCH["w"])[-1])
    assert cap >= n
    out = [np.zeros(cap, np.uint64), np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(off.size, np.uint64)]
    assert raw(ctx, bases, off, out[0], out[1], out[2], out[3], cap, out[4]) == (A.OK, n)
    same([x[:n] for x in out[:4]] + [out[4]], want)


def test_every_combination_of_optional_outputs(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    for use in itertools.product((False, True), repeat=4):
        out = [np.zeros(n, np.uint64)] + [np.zeros(n, t) if u else None for u, t in zip(use[:3], (np.uint32, np.uint32, np.uint8))]
        out.append(np.zeros(off.size, np.uint64) if use[3] else None)
        assert raw(ctx, bases, off, out[0], out[1], out[2], out[3], n, out[4]) == (A.OK, n), use
        for g, x in zip(out, want):
            assert g is None or np.array_equal(g, x), use


def test_two_calls_give_identical_arrays(ctx, oracle):
    reads = rand_reads(10, [5 * T + 17, 40, 900])
    bases, off = oracle.concat(reads)
    a = ctx.read_minimizers(bases, off, A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, 19)
    b = ctx.read_minimizers(bases, off, A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, 19)
    same(a, b)


def test_no_read_and_no_kmer(ctx):
    off = np.zeros(1, np.uint64)
    moff = np.full(1, 9, np.uint64)
    assert raw(ctx, np.zeros(16, np.uint8), off, None, None, None, None, 0, moff) == (A.OK, 0) and moff[0] == 0
    got = ctx.read_minimizers(np.frombuffer(b"ACGTACGTAC" + b"A" * 6, np.uint8).copy(), np.array([0, 4, 4, 10], np.uint64), A.KMER64BIT, 21,
                              A.FHASH_CANON_INVHASH, 10)
    assert got[0].size == 0 and got[4].tolist() == [0, 0, 0, 0]


def test_a_batch_of_empty_reads_on_host_and_device_arrays(ctx):
    """reads but no base at all: an empty tensor has no address, and the binding must not hand the library a null pointer for it"""
    import torch
    off = np.zeros(4, np.uint64)
    got = ctx.read_minimizers(np.zeros(0, np.uint8), off, A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, 10)
    assert [x.shape for x in got] == [(0,)] * 4 + [(4,)] and got[4].tolist() == [0, 0, 0, 0]
    d = ctx.read_minimizers(torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), A.KMER64BIT, 21,
                            A.FHASH_CANON_INVHASH, 10)
    assert all(x.is_cuda for x in d) and [tuple(x.shape) for x in d] == [(0,)] * 4 + [(4,)] and d[4].cpu().tolist() == [0, 0, 0, 0]
    m = minimizer.read_minimizers(ctx, torch.zeros(0, dtype=torch.uint8, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), 15, 10)
    assert minimizer.seed_pairs(ctx, m).shape[0] == 0


# ---- errors ---------------------------------------------------------------------------------------------------------------------
def test_non_acgt_is_reported_and_does_not_stick(ctx, oracle):
    k, w = 21, 10
    reads = rand_reads(12, [400, 2 * T + 300, 15])
    spots = [(0, 100), (1, T + 50 + k - 1), (1, len(reads[1]) - 1), (2, 3), (0, 0)]  # the last base of a read; a read shorter than k
    for r, p in spots:
        bad = [bytearray(s) for s in reads]
        bad[r][p] = ord("N")
        bases, off = oracle.concat([bytes(s) for s in bad])
        with pytest.raises(lib.KmuError) as e:
            ctx.read_minimizers(bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)
        assert e.value.code == A.E_NON_ACGT, (r, p)
        check(ctx, oracle, reads, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w)  # the next call is clean


def test_refused_arguments(ctx, batch):
    bases, off, want = batch
    n = want[0].size
    hashes, strand = np.zeros(n, np.uint64), np.zeros(n, np.uint8)
    assert raw(ctx, bases, off, hashes, None, None, None, n, None, kmer_type=A.KMERAA32BIT)[0] == A.E_BAD_ALPHABET
    assert raw(ctx, bases, off, hashes, None, None, None, n, None, input_kind=A.INPUT_PACKED2)[0] == A.E_UNSUPPORTED
    assert raw(ctx, bases, off, hashes, None, None, None, n, None, w=0)[0] == A.E_BAD_ARG
    assert raw(ctx, bases, off, hashes, None, None, None, n, None, w=MAX_W + 1)[0] == A.E_UNSUPPORTED
    assert raw(ctx, bases, off, hashes, None, None, None, n, None, mem=7)[0] == A.E_BAD_ARG
    assert raw(ctx, bases, off, hashes, None, None, strand, n, None, fhash=A.FHASH_CANON_NTHASH)[0] == A.E_UNSUPPORTED
    assert raw(ctx, bases, off, None, None, None, None, 0, None, fhash=A.FHASH_CANON_NTHASH)[0] == A.OK
    assert raw(ctx, bases, off, None, None, None, None, 0, None, kmer_type=A.KMER32BIT)[0] == A.E_BAD_K  # k = 21: as kmu_kmer_hashes
    hp = A.HashParams(A.KMER64BIT, 21, A.FHASH_CANON_INVHASH, A.INPUT_ASCII, A.MEM_HOST, 0)
    P = lambda x: lib._ptr(x)[0]  # noqa: E731
    assert ctx.L.kmu_read_minimizers(ctx.h, C.byref(hp), P(bases), P(off), off.size - 1, 10, None, None, None, None, 0, None, None) == A.E_BAD_ARG
    assert ctx.L.kmu_read_minimizers(ctx.h, None, P(bases), P(off), off.size - 1, 10, None, None, None, None, 0, None, C.byref(C.c_uint64())) == A.E_BAD_ARG
    same(ctx.read_minimizers(bases, off, BATCH["kmer_type"], BATCH["k"], BATCH["fhash"], BATCH["w"]), want)  # and the context still works


# ---- seed hits ------------------------------------------------------------------------------------------------------------------
def reference_hits(q, db, own, max_occ):
    """a dict join over the host arrays: the set of (read_a, pos_a, strand_a, read_b, pos_b, strand_b)"""
    by_hash = {}
    for h, r, p, s in zip(db.hashes.tolist(), db.read.tolist(), db.pos.tolist(), db.strand.tolist()):
        by_hash.setdefault(h, []).append((r, p, s))
    hits = set()
    for h, r, p, s in zip(q.hashes.tolist(), q.read.tolist(), q.pos.tolist(), q.strand.tolist()):
        bucket = by_hash.get(h, ())
        if max_occ and len(bucket) > max_occ:
            continue
        for (r2, p2, s2) in bucket:
            if not own or r2 != r:
                hits.add((r, p, s, r2, p2, s2))
    return hits


def test_seed_hits(ctx, oracle):
    import torch
    k, w = 21, 19
    genome = rand_reads(13, [50000])[0]
    starts = np.linspace(0, 48000, 200).astype(int)
    reads = [genome[b:b + 2000] for b in starts] + [revcomp(genome[b:b + 2000]) for b in starts[[3, 50, 120]]]
    bases, off = oracle.concat(reads)
    q = minimizer.read_minimizers(ctx, bases, off, k, w)
    same(q[:5], expected(oracle, bases, off, A.KMER64BIT, k, A.FHASH_CANON_INVHASH, w))
    got = minimizer.seed_hits(ctx, q)
    want = reference_hits(q, q, True, 0)
    assert got.dtype == np.int64 and got.shape == (len(want), 6) and set(map(tuple, got.tolist())) == want
    assert any(a[2] != a[5] for a in want)  # the opposite-strand copies hit on opposite strands
    # on the device, with a repeat mask
    d_bases, d_off = torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda()
    dq = minimizer.read_minimizers(ctx, d_bases, d_off, k, w)
    got = minimizer.seed_hits(ctx, dq, max_occ=6)
    want_masked = reference_hits(q, q, True, 6)
    assert got.is_cuda and 0 < len(want_masked) < len(want)
    assert tuple(got.shape) == (len(want_masked), 6) and set(map(tuple, got.cpu().tolist())) == want_masked
    # a database of its own: reads are numbered per batch, every equal hash is a hit
    sub_bases, sub_off = oracle.concat(reads[10:14])
    db = minimizer.read_minimizers(ctx, sub_bases, sub_off, k, w)
    got = minimizer.seed_hits(ctx, q, db)
    want_db = reference_hits(q, db, False, 0)
    assert got.shape == (len(want_db), 6) and set(map(tuple, got.tolist())) == want_db

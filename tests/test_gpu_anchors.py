"""-m gpu: kmu_read_anchors against the oracle.  The expected row of every slice is oracle.sketch (bottom-k, counts) of the
substring seq[beg:end] as a sequence of its own; beg / end are computed here from the rules of the reference (anchor.rs:242,
295-318), not from the library's layout:  stride = window - overlap, one slice per beg = s * stride < L,
end = min(beg + window, L - 1).  (tests/test_anchor_abi.py checks on the CPU what this relies on in the oracle.)"""
import json
import os

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXH = np.uint64(0xFFFFFFFFFFFFFFFF)
T = A.ANCHOR_TILE_KMERS
REF = (A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED)  # the reference's own anchors
CANON = (A.HASHER_INT64HASH, A.FHASH_CANON_VALUE)
NOHASH = (A.HASHER_NOHASH, A.FHASH_CANON_INVHASH)


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def params(kmer_type, k, m, hf, algo=A.ALGO_BOTTOMK, block_size=0, input_kind=A.INPUT_ASCII):
    return A.SketchParams(algo, kmer_type, k, m, A.SIG_U64, hf[0], hf[1], block_size, A.MODE_PER_SEQ, input_kind, A.MEM_HOST, 0)


def rand_reads(seed, lens):
    rng = np.random.default_rng(seed)
    return [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(n))) for n in lens]


def expected(oracle, reads, p, window, overlap):
    """(hashes, counts, n, row_offsets) by the rules above; one oracle call over all non-empty substrings"""
    stride = window - overlap
    subs, row_off = [], [0]
    for s in reads:
        L = len(s)
        beg = 0
        while beg < L:
            subs.append(s[beg:min(beg + window, L - 1)])
            beg += stride
        row_off.append(len(subs))
    m = p.sketch_size
    hashes = np.full((len(subs), m), MAXH, np.uint64)
    counts = np.zeros((len(subs), m), np.uint32)
    full = [i for i, s in enumerate(subs) if len(s)]  # (an empty substring is no sequence for the oracle: its row is all padding)
    if full:
        bases, off = oracle.concat([subs[i] for i in full])
        h, c = oracle.sketch(bases, off, p, want_counts=True)
        hashes[full], counts[full] = h, c
    n = (hashes != MAXH).sum(axis=1).astype(np.uint32)
    return hashes, counts, n, np.array(row_off, np.uint64)


def check(ctx, oracle, reads, p, window, overlap):
    bases, off = oracle.concat(reads)
    got = ctx.read_anchors(bases, off, p, window, overlap)
    want = expected(oracle, reads, p, window, overlap)
    assert np.array_equal(got[3], want[3]), "row_offsets"
    assert got[0].shape == want[0].shape
    bad = np.nonzero((got[0] != want[0]).any(axis=1) | (got[1] != want[1]).any(axis=1) | (got[2] != want[2]))[0]
    assert bad.size == 0, "rows %s differ; first: got %s / %s n %s, want %s / %s n %s" % (
        bad[:8].tolist(), got[0][bad[0]], got[1][bad[0]], got[2][bad[0]], want[0][bad[0]], want[1][bad[0]], want[2][bad[0]])
    return got


@pytest.mark.parametrize("hf", [REF, CANON, NOHASH], ids=["int64hash_value", "int64hash_canon", "nohash_caninv"])
@pytest.mark.parametrize("kmer_type,k", [(A.KMER32BIT, 11), (A.KMER16B32BIT, 16), (A.KMER64BIT, 21), (A.KMER64BIT, 31)])
def test_parity(ctx, oracle, kmer_type, k, hf):
    lens = np.random.default_rng(k).integers(1, 3001, size=40)
    check(ctx, oracle, rand_reads(100 + k, lens), params(kmer_type, k, 16, hf), 500, 125)


def test_slice_rule_edges(ctx, oracle):
    k, window, overlap = 21, 100, 25
    stride = window - overlap
    p = params(A.KMER64BIT, k, 8, REF)
    lens = [3 * stride, 3 * stride + 1, 3 * stride + 2, 1, k - 1, k, k + 1, k + 2, 60, window, window + 1, 5 * stride + 1]
    got = check(ctx, oracle, rand_reads(1, lens), p, window, overlap)
    rows = got[3]
    assert got[2][int(rows[2]) - 1] == 0  # L = 3 stride + 1: the last slice is beg == end, an empty row (the reference panics)
    assert int(rows[2] - rows[1]) == 4 and int(rows[1] - rows[0]) == 3


def test_window_shorter_than_k_gives_empty_rows(ctx, oracle):
    got = check(ctx, oracle, rand_reads(2, [5, 64, 300]), params(A.KMER64BIT, 21, 4, REF), 20, 5)
    assert (got[2] == 0).all() and (got[0] == MAXH).all() and (got[1] == 0).all()


@pytest.mark.parametrize("window,overlap", [(120, 0), (64, 63), (60, 23), (500, 499)])
def test_overlaps_and_unaligned_strides(ctx, oracle, window, overlap):
    """overlap 0; overlap window - 1 (one slice per base) on one read of 300 bases; stride 37: slices that start at no multiple of
    4 or 16"""
    lens = [300] if overlap == window - 1 else [300, 411, 37, 38, 75]
    check(ctx, oracle, rand_reads(3, lens), params(A.KMER64BIT, 21, 16, CANON), window, overlap)


def test_batch_that_starts_inside_a_larger_array(ctx, oracle):
    """offsets + first of a larger array: offsets[0] != 0, on the host and on the device"""
    import torch
    reads = rand_reads(4, [333, 700, 41, 1200, 515, 90])
    p = params(A.KMER64BIT, 21, 16, REF)
    bases, off = oracle.concat(reads)
    first, last = 2, 5
    want = expected(oracle, reads[first:last], p, 200, 50)
    got = ctx.read_anchors(bases, off[first:last + 1].copy(), p, 200, 50)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    d_bases = torch.from_numpy(bases).cuda()
    d_off = torch.from_numpy(off.astype(np.int64)).cuda()
    gd = ctx.read_anchors(d_bases, d_off[first:last + 1], p, 200, 50)
    for g, w in zip(gd[:3], want[:3]):
        assert np.array_equal(anchor._host(g), w)
    assert np.array_equal(gd[3], want[3])


@pytest.mark.parametrize("m", [1, 16, A.ANCHOR_MAX_NBKMER])
@pytest.mark.parametrize("nk", [T - 1, T, T + 1, 2 * T + 1])
def test_tile_boundaries(ctx, oracle, nk, m):
    """one read whose (only full) window holds exactly nk k-mers: window = nk + k - 1, the read one base longer"""
    k = 21
    window = nk + k - 1
    reads = rand_reads(nk, [window + 1]) + rand_reads(nk + 1, [window + 40])
    check(ctx, oracle, reads, params(A.KMER64BIT, k, m, REF), window, 10)


def test_padding_when_nbkmer_exceeds_the_distinct_kmers(ctx, oracle):
    k, m = 11, A.ANCHOR_MAX_NBKMER
    reads = [b"ACGT" * 250, rand_reads(9, [120])[0], b"AC" * ((2 * T + 40) // 2)]  # 4 / 110 / 2 distinct k-mers, the last over three tiles
    got = check(ctx, oracle, reads, params(A.KMER32BIT, k, m, CANON), 2 * T + 30, 100)
    assert got[2].max() < m and (got[0][:, -1] == MAXH).all()


@pytest.mark.parametrize("hf", [REF, NOHASH], ids=["int64hash_wraps", "nohash_u16"])
def test_multiplicities(ctx, oracle, hf):
    """poly-A windows of 255, 256 and 301 k-mers (u8 counts wrap under INT64HASH: 255, 0, 45; u16 counts do not), and a tandem
    repeat longer than two tiles, whose counts are summed across tiles"""
    k = 21
    p = params(A.KMER64BIT, k, 4, hf)
    for nk in (255, 256, 301):
        window = nk + k - 1
        got = check(ctx, oracle, [b"A" * (window + 1)], p, window, 0)
        assert got[1][0, 0] == (nk & 0xFF if hf is REF else nk) and got[2][0] == 1
    window = 2 * T + 300
    got = check(ctx, oracle, [b"ACGT" * ((window + 4) // 4)], p, window, 7)
    nk = window - k + 1
    per_phase = [(nk - j + 3) // 4 for j in range(4)]  # occurrences of the k-mer that starts at phase j of the repeat
    if hf is REF:  # forward k-mers: four distinct ones, u8 counts
        want = sorted(c & 0xFF for c in per_phase)
    else:  # canonical k-mers: ACGT is its own reverse complement, phases 0 / 3 and 1 / 2 are one k-mer each; u16 counts
        want = sorted([per_phase[0] + per_phase[3], per_phase[1] + per_phase[2]])
    n = int(got[2][0])
    assert n == len(want) and sorted(got[1][0][:n].tolist()) == want


def test_device_buffers_give_the_same_arrays(ctx, oracle):
    import torch
    reads = rand_reads(6, np.random.default_rng(6).integers(1, 2500, size=30))
    p = params(A.KMER64BIT, 21, 16, CANON)
    bases, off = oracle.concat(reads)
    host = check(ctx, oracle, reads, p, 500, 125)
    dev = ctx.read_anchors(torch.from_numpy(bases).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), p, 500, 125)
    assert dev[0].is_cuda and dev[1].is_cuda and dev[2].is_cuda
    for d, h in zip(dev[:3], host[:3]):
        assert np.array_equal(anchor._host(d), h)
    assert np.array_equal(dev[3], host[3])


def test_optional_outputs(ctx, oracle):
    """counts_out / n_out NULL in every combination, through the C-ABI"""
    import ctypes as C
    reads = rand_reads(7, [700, 50, 1301])
    p = params(A.KMER64BIT, 21, 16, REF)
    bases, off = oracle.concat(reads)
    want = expected(oracle, reads, p, 300, 100)
    rows = int(want[3][-1])
    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    for with_counts in (False, True):
        for with_n in (False, True):
            h = np.zeros((rows, 16), np.uint64)
            c = np.full((rows, 16), 7, np.uint32) if with_counts else None
            n = np.full(rows, 7, np.uint32) if with_n else None
            rc = ctx.L.kmu_read_anchors(ctx.h, C.byref(p), vp(bases), vp(off), 3, 300, 100, vp(want[3]), vp(h), vp(c), vp(n))
            assert rc == 0
            assert np.array_equal(h, want[0])
            assert c is None or np.array_equal(c, want[1])
            assert n is None or np.array_equal(n, want[2])
    hashes, counts, n, _ = ctx.read_anchors(bases, off, p, 300, 100, want_counts=False)
    assert counts is None and np.array_equal(hashes, want[0]) and np.array_equal(n, want[2])


def test_nothing_to_do(ctx, oracle):
    import ctypes as C
    p = params(A.KMER64BIT, 21, 16, REF)
    zero = np.zeros(1, np.uint64)
    assert ctx.L.kmu_read_anchors(ctx.h, C.byref(p), None, zero.ctypes.data_as(C.c_void_p), 0, 100, 10, None, None, None, None) == 0
    bases, off = oracle.concat([b"", b""])
    got = ctx.read_anchors(bases, off, p, 100, 10)  # reads of L = 0: no rows, no error
    assert got[0].shape == (0, 16) and got[3].tolist() == [0, 0, 0]


def _code(ctx, *args, **kw):
    with pytest.raises(lib.KmuError) as e:
        ctx.read_anchors(*args, **kw)
    return e.value.code


def test_errors(ctx, oracle):
    import ctypes as C
    reads = rand_reads(8, [400, 300, 250])
    bases, off = oracle.concat(reads)
    ok = params(A.KMER64BIT, 21, 16, REF)
    for pos in (137, 299):  # 299: the last base of a read lies in no anchor; the read is refused all the same
        nb = bytearray(reads[1])
        nb[pos] = ord("N")
        b2, o2 = oracle.concat([reads[0], bytes(nb), reads[2]])
        assert _code(ctx, b2, o2, ok, 100, 25) == A.E_NON_ACGT
    ctx.read_anchors(bases, off, ok, 100, 25)  # the error word does not stick to the next call
    aa, oa = oracle.concat([b"MTEQIELIKLYSTRILALAAQMPHVGSLDNPDASAMKRSPLC"])
    assert _code(ctx, aa, oa, params(A.KMERAA32BIT, 5, 16, (A.HASHER_NOHASH, A.FHASH_VALUE_MASKED)), 20, 5) == A.E_BAD_ALPHABET
    assert _code(ctx, bases, off, params(A.KMER64BIT, 21, 16, (A.HASHER_NOHASH, A.FHASH_CANON_INVHASH), algo=A.ALGO_PROB3A), 100, 25) == A.E_BAD_ARG
    assert _code(ctx, bases, off, params(A.KMER64BIT, 21, 16, REF, block_size=100), 100, 25) == A.E_BAD_ARG
    assert _code(ctx, bases, off, params(A.KMER64BIT, 21, A.ANCHOR_MAX_NBKMER + 1, REF), 100, 25) == A.E_UNSUPPORTED
    assert _code(ctx, bases, off, params(A.KMER64BIT, 21, 16, REF, input_kind=A.INPUT_PACKED2), 100, 25) == A.E_UNSUPPORTED
    for window, overlap in ((0, 0), (100, 100), (10, 30)):
        assert _code(ctx, bases, off, ok, window, overlap) == A.E_BAD_ARG
    # a wrong anchor_row_offsets (host): refused before any kernel runs, outputs untouched
    rows = lib.anchor_layout(off, 100, 25)
    wrong = rows.copy()
    wrong[1] += 1
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = np.full((int(rows[-1]) + 1, 16), 3, np.uint64)
    c = np.full((int(rows[-1]) + 1, 16), 3, np.uint32)
    n = np.full(int(rows[-1]) + 1, 3, np.uint32)
    assert ctx.L.kmu_read_anchors(ctx.h, C.byref(ok), vp(bases), vp(off), 3, 100, 25, vp(wrong), vp(h), vp(c), vp(n)) == A.E_BAD_ARG
    assert (h == 3).all() and (c == 3).all() and (n == 3).all()


def test_python_mirror_on_the_reference_sequence(ctx, oracle):
    with open(os.path.join(ROOT, "tests", "golden", "reference_kats.json")) as f:
        seq = json.load(f)["seq80"].encode()
    ap = anchor.AnchorsGeneratorParameters("seq80.fasta", 30, 4, 11, 10)
    bases, off = oracle.concat([seq])
    ras = anchor.gen_read_anchors(ctx, bases, off, ap, first_readnum=3)
    assert len(ras) == 1 and ras[0].readnum == 3
    assert ras[0].get_nb_slice() == 4 and [s.slicepos for s in ras[0].anchors] == [0, 20, 40, 60]
    want = expected(oracle, [seq], ap.sketch_params(), 30, 10)
    for r, s in enumerate(ras[0].anchors):
        assert s.minhash == [(int(want[0][r, t]), int(want[1][r, t])) for t in range(int(want[2][r]))]
    hashes, counts, n, rows = ctx.read_anchors(bases, off, ap.sketch_params(), 30, 10)
    idx = anchor.anchors_by_minhash(hashes, n, rows, ap.get_stride(), first_readnum=3)
    nonempty = [r for r in range(4) if n[r] > 0]
    assert sorted(idx) == sorted({int(hashes[r, 0]) for r in nonempty})
    assert sorted(v for vs in idx.values() for v in vs) == [(3, 20 * r) for r in nonempty]

"""Reading the count table back: kmu_count_histogram (the count spectrum) and kmu_count_read_profile (the abundance of the k-mers
of reads: per position, and summarised per read).  No counterpart upstream; every expected value is stated with the oracle's
counter -- want = min(oracle 16-bit count of the canonical k-mer, 2^bits - 1) -- and numpy, and compared for equality."""
import os

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

pytestmark = pytest.mark.gpu

DT = np.dtype(A.READ_ABUNDANCE_DTYPE)
SHORT_MAX = 4096  # PROFILE_SHORT_MAX of kmu_count_read.hip: one wave per read up to this many k-mers, the block above


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _cat(parts):
    bases = np.concatenate([b for b, _ in parts])
    lens = np.concatenate([np.diff(o.astype(np.int64)) for _, o in parts])
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return bases, off


def added_reads():
    """120 reads of 300 bases of a 20 kb genome with 1 % substitutions, and a poly-A read of 2 500 bases: 2 470 occurrences of one
    31-mer (beyond 255 and beyond the smallest quotient count field)"""
    b, o = synth.genome_reads(120, np.full(120, 300, np.int64), 20_000, 0xA1, sub=0.01)
    poly = np.frombuffer(b"A" * 2500, np.uint8)
    return _cat([(b, o), (poly, np.array([0, 2500], np.uint64))])


def query_reads(k):
    """not the reads added: half from the genome of the added reads, half from another one (absent k-mers), lengths that cross the
    units of the walk (a wave step is 1 024 bases of the flat stream) and of the statistics kernel"""
    lens = [k - 1, k, k + 1] + list(range(31, 41)) * 3 + [1023, 1024, 1025, 5000]
    lens += [SHORT_MAX + k - 2, SHORT_MAX + k - 1, SHORT_MAX + k]  # SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1 k-mers
    tot = sum(lens) + 300
    lens += [300 + (-tot) % 1024, 35]  # a read that ends exactly on a step boundary, then a short one
    assert sum(lens[:-1]) % 1024 == 0
    lens = np.array(lens, np.int64)
    own = synth.genome_reads(lens.size, lens, 20_000, 0xA1, sub=0.01)
    other = synth.genome_reads(lens.size, lens, 20_000, 0xB2)
    bases, off = own[0].copy(), own[1]
    for i in range(1, lens.size, 2):
        bases[int(off[i]):int(off[i + 1])] = other[0][int(off[i]):int(off[i + 1])]
    # counts above 255 inside reads that also hold counts below 256: runs of A in the 5 000-base read and in a short one
    i5 = int(np.flatnonzero(lens == 5000)[0])
    bases[int(off[i5]) + 1000:int(off[i5]) + 3800] = ord("A")
    i300 = lens.size - 2
    bases[int(off[i300]) + 40:int(off[i300]) + 140] = ord("A")
    return bases, off


def expected(oracle, ocounter, bases, off, ktype, k, bits, solid_min):
    canon = oracle.kmer_hashes(bases, off, ktype, k, A.FHASH_CANON_VALUE)
    q = np.minimum(ocounter.query(canon), (1 << bits) - 1).astype(np.uint16)
    counts = np.zeros(int(off[-1]), np.uint16)
    stats = np.zeros(off.size - 1, DT)
    for i in range(off.size - 1):
        b, L = int(off[i]), int(off[i + 1]) - int(off[i])
        n = max(L - k + 1, 0)
        c = q[b:b + n]
        counts[b:b + n] = c
        if n:
            stats[i] = (n, (c == 0).sum(), (c == 1).sum(), (c >= solid_min).sum(), c.min(), np.sort(c)[(n - 1) // 2], c.max(), 0,
                        c.astype(np.uint64).sum())
    return counts, stats


_CASES = {}


def case(oracle, ktype, k):
    """(added reads, oracle counter, query reads): computed once per k-mer type, shared, never changed"""
    if (ktype, k) not in _CASES:
        ab, ao = added_reads()
        o = oracle.Counter(ktype, k, 16, 1 << 20)
        o.add_reads(ab, ao)
        _CASES[(ktype, k)] = (ab, ao, o, query_reads(k))
    return _CASES[(ktype, k)]


def dev(x):
    import torch
    return torch.from_numpy(x.astype(np.int64) if x.dtype == np.uint64 else x).cuda()


def dev_stats(t):
    return t.cpu().numpy().view(DT).reshape(-1)


# ---- the histogram -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regions", ["1", "3", "2052"])
@pytest.mark.parametrize("fmt", ["wide", "quot"])
@pytest.mark.parametrize("bits", [8, 16])
def test_histogram(ctx, oracle, monkeypatch, bits, fmt, regions):
    import torch
    monkeypatch.setenv("KMU_COUNT_FMT", fmt)
    monkeypatch.setenv("KMU_COUNT_REGIONS", regions)
    ab, ao, o, _ = case(oracle, A.KMER64BIT, 31)
    if regions in ("1", "3"):  # one / three regions of 4 096 slots only hold so much
        nr = 8 if regions == "1" else 24
        ab, ao = ab[:int(ao[nr])], ao[:nr + 1]
        ab, ao = _cat([(ab, ao), (np.frombuffer(b"A" * 2500, np.uint8), np.array([0, 2500], np.uint64))])
        o = oracle.Counter(A.KMER64BIT, 31, 16, 1 << 16)
        o.add_reads(ab, ao)
    maxc = (1 << bits) - 1
    _, wc = o.dump(1)
    wc = np.minimum(wc, maxc).astype(np.int64)
    assert wc.max() == min(2470, maxc)
    c = ctx.counter(A.KMER64BIT, 31, bits, 1024)
    c.add_reads(ab, ao)
    for n_bins in (2, 3, 256, 257, 65536):
        want = np.bincount(np.minimum(wc, n_bins - 1), minlength=n_bins).astype(np.uint64)
        got = c.histogram(n_bins)
        assert got.dtype == np.uint64 and got.size == n_bins
        assert np.array_equal(got, want), (bits, fmt, regions, n_bins)
        assert got[0] == 0 and int(got.sum()) == o.nb_distinct() == c.nb_distinct()
        if n_bins > 2:
            assert int(got[1]) == o.nb_unique() == c.nb_unique()
        gd = c.histogram(n_bins, device=torch.device("cuda", 0))  # device output memory
        assert np.array_equal(gd.cpu().numpy().astype(np.uint64), want)
    full = c.histogram()
    assert full.size == 1 << bits
    if bits == 16:
        assert int((np.arange(full.size, dtype=np.uint64) * full).sum()) == c.nb_occurrences()
    c.close()


def test_histogram_edges(ctx, oracle, monkeypatch):
    from kmerutils_amd import lib
    ab, ao, o, _ = case(oracle, A.KMER64BIT, 31)
    _, wc = o.dump(1)
    # an empty counter, and one whose table waits for its first add
    for kw in ({}, {"hint_occurrences": True}):
        c = ctx.counter(A.KMER64BIT, 31, 8, 1 << 16, **kw)
        assert not c.histogram().any() and c.histogram().size == 256
        c.close()
    # after eliminate_once
    c = ctx.counter(A.KMER64BIT, 31, 16, 1 << 16)
    c.add_reads(ab, ao)
    c.eliminate_once()
    h = c.histogram()
    assert h[1] == 0 and np.array_equal(h, np.bincount(wc[wc >= 2], minlength=65536).astype(np.uint64))
    # n_bins outside [2, 65536]
    for bad in (0, 1, 65537):
        with pytest.raises(lib.KmuError) as e:
            c.histogram(bad)
        assert e.value.code == A.E_BAD_ARG
    c.close()


def test_histogram_world1_distributed(oracle, monkeypatch):
    from kmerutils_amd import lib
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", os.environ.get("NCCL_SOCKET_IFNAME", "lo"))
    ab, ao, o, (qb, qo) = case(oracle, A.KMER64BIT, 31)
    _, wc = o.dump(1)
    ctx = lib.Context(0)
    ctx.comm_init(lib.Context.comm_get_id(), 0, 1)
    c = ctx.counter(A.KMER64BIT, 31, 16, 1 << 16, distributed=True)
    c.add_reads(ab, ao)
    c.finalize()
    assert np.array_equal(c.histogram(), np.bincount(wc, minlength=65536).astype(np.uint64))
    # one rank holds every key: the profile answers too
    wcnt, wst = expected(oracle, o, qb, qo, A.KMER64BIT, 31, 16, 2)
    gc, gs = c.read_profile(qb, qo)
    assert np.array_equal(gc, wcnt) and np.array_equal(gs, wst)
    c.close()
    ctx.comm_destroy()
    ctx.close()


# ---- the profile -------------------------------------------------------------------------------------------------------------
KMERS = [(A.KMER32BIT, 8), (A.KMER16B32BIT, 16), (A.KMER64BIT, 17), (A.KMER64BIT, 31)]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("ktype,k", KMERS, ids=["k8", "k16", "k17", "k31"])
def test_profile_counts_and_stats(ctx, oracle, ktype, k, bits):
    """per-position counts and the records, host and device memory, every combination of the two outputs"""
    ab, ao, o, (qb, qo) = case(oracle, ktype, k)
    wcnt, wst = expected(oracle, o, qb, qo, ktype, k, bits, 2)
    assert wst["n_absent"].sum() > 0 and (wst["n_kmers"][:3] == [0, 1, 2]).all()
    if bits == 16:  # both median rounds: counts above 255 and below 256 in one read, the median on either side
        mixed = (wst["max"] > 255) & (wst["min"] < 256)
        assert (mixed & (wst["median"] > 255)).any() and (mixed & (wst["median"] < 256)).any()
    c = ctx.counter(ktype, k, bits, 1 << 16)
    c.add_reads(ab, ao)
    # host
    gc, gs = c.read_profile(qb, qo)
    assert gc.dtype == np.uint16 and np.array_equal(gc, wcnt)  # (the last k - 1 positions of every read: zero)
    assert np.array_equal(gs, wst)
    assert np.array_equal(c.read_profile(qb, qo, want_counts=False), wst)
    assert np.array_equal(c.read_profile(qb, qo, want_stats=False), wcnt)
    # into an array that held something else: host arrays come back whole
    assert np.array_equal(c.read_profile(qb, qo, want_stats=False, counts_out=np.full(int(qo[-1]), 0x5A5A, np.uint16)), wcnt)
    # device: the positions that start no k-mer keep what the array held
    import torch
    db, do = dev(qb), dev(qo)
    valid = np.zeros(int(qo[-1]), bool)
    for i in range(qo.size - 1):
        valid[int(qo[i]):int(qo[i]) + max(int(qo[i + 1]) - int(qo[i]) - k + 1, 0)] = True
    sent = torch.full((int(qo[-1]),), 0x5A5A, dtype=torch.int16, device="cuda")
    dc, dst = c.read_profile(db, do, counts_out=sent)
    dc = dc.cpu().numpy().view(np.uint16)
    assert np.array_equal(dc[valid], wcnt[valid]) and (dc[~valid] == 0x5A5A).all()
    assert np.array_equal(dev_stats(dst), wst)
    assert np.array_equal(dev_stats(c.read_profile(db, do, want_counts=False)), wst)
    c.close()


def test_profile_subrange_view(ctx, oracle):
    """`offsets + first` of a larger read set: offsets[0] != 0, counts at the caller's indices"""
    import torch
    ktype, k = A.KMER64BIT, 31
    ab, ao, o, (qb, qo) = case(oracle, ktype, k)
    wcnt, wst = expected(oracle, o, qb, qo, ktype, k, 16, 2)
    c = ctx.counter(ktype, k, 16, 1 << 16)
    c.add_reads(ab, ao)
    db, do = dev(qb), dev(qo)
    for first, last in ((5, 30), (34, qo.size - 1), (36, 38)):  # (36: the 5 000-base read, past the first wave steps)
        lo, hi = int(qo[first]), int(qo[last])
        gc, gs = c.read_profile(qb, qo[first:last + 1], counts_out=np.full(int(qo[-1]), 0x5A5A, np.uint16))
        assert np.array_equal(gc[lo:hi], wcnt[lo:hi]) and (gc[:lo] == 0x5A5A).all() and (gc[hi:] == 0x5A5A).all()
        assert np.array_equal(gs, wst[first:last])
        sent = torch.full((int(qo[-1]),), 0x5A5A, dtype=torch.int16, device="cuda")
        dc, dst = c.read_profile(db, do[first:last + 1], counts_out=sent)
        dc = dc.cpu().numpy().view(np.uint16)
        want = np.full(int(qo[-1]), 0x5A5A, np.uint16)
        for i in range(first, last):
            n = max(int(qo[i + 1]) - int(qo[i]) - k + 1, 0)
            want[int(qo[i]):int(qo[i]) + n] = wcnt[int(qo[i]):int(qo[i]) + n]
        assert np.array_equal(dc, want), (first, last)
        assert np.array_equal(dev_stats(dst), wst[first:last])
        assert np.array_equal(dev_stats(c.read_profile(db, do[first:last + 1], want_counts=False)), wst[first:last])
    c.close()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("short_max", [None, "33", "1000000"])
def test_profile_both_read_shapes(ctx, oracle, monkeypatch, bits, short_max):
    """one wave per read up to PROFILE_SHORT_MAX k-mers, the block above: the query reads hold SHORT_MAX - 1, SHORT_MAX and
    SHORT_MAX + 1 k-mers (and 5 000 bases); KMU_PROFILE_SHORT_MAX moves the length: nearly every read by the block, every read by
    a wave"""
    ktype, k = A.KMER64BIT, 31
    ab, ao, o, (qb, qo) = case(oracle, ktype, k)
    nk = np.diff(qo.astype(np.int64)) - k + 1
    assert all(v in nk for v in (SHORT_MAX - 1, SHORT_MAX, SHORT_MAX + 1))
    if short_max:
        monkeypatch.setenv("KMU_PROFILE_SHORT_MAX", short_max)
    c = ctx.counter(ktype, k, bits, 1 << 16)
    c.add_reads(ab, ao)
    for solid_min in (1, 2, 300):
        _, wst = expected(oracle, o, qb, qo, ktype, k, bits, solid_min)
        assert np.array_equal(c.read_profile(qb, qo, solid_min, want_counts=False), wst), solid_min
        assert np.array_equal(c.read_profile(qb, qo, solid_min)[1], wst), solid_min
    c.close()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("chunk", ["2048", "4096", "6000"])
def test_profile_bounded_workspace(ctx, oracle, monkeypatch, bits, chunk):
    """statistics alone pass the counts through a workspace of KMU_PROFILE_CHUNK counts: several chunks of whole reads, and reads
    longer than a chunk (4 125 .. 5 000 bases against 2 048 and 4 096) taken over sub-ranges -- the records of the unchunked call"""
    ktype, k = A.KMER64BIT, 31
    ab, ao, o, (qb, qo) = case(oracle, ktype, k)
    _, wst = expected(oracle, o, qb, qo, ktype, k, bits, 2)
    monkeypatch.setenv("KMU_PROFILE_CHUNK", chunk)
    c = ctx.counter(ktype, k, bits, 1 << 16)
    c.add_reads(ab, ao)
    assert np.array_equal(c.read_profile(qb, qo, want_counts=False), wst)
    assert np.array_equal(dev_stats(c.read_profile(dev(qb), dev(qo), want_counts=False)), wst)
    assert np.array_equal(dev_stats(c.read_profile(dev(qb), dev(qo)[30:], want_counts=False)), wst[30:])
    c.close()


def test_profile_edges(ctx, oracle):
    from kmerutils_amd import lib
    ktype, k = A.KMER64BIT, 31
    ab, ao, o, (qb, qo) = case(oracle, ktype, k)
    # an empty counter: every k-mer absent
    c = ctx.counter(ktype, k, 8, 1 << 16)
    gc, gs = c.read_profile(qb, qo)
    n = np.maximum(np.diff(qo.astype(np.int64)) - k + 1, 0)
    assert not gc.any() and np.array_equal(gs["n_kmers"], n) and np.array_equal(gs["n_absent"], n)
    assert not (gs["n_once"].any() or gs["n_solid"].any() or gs["max"].any() or gs["sum"].any())
    c.add_reads(ab, ao)
    # a read with an N
    bad = qb[:2000].copy()
    bad[777] = ord("N")
    with pytest.raises(lib.KmuError) as e:
        c.read_profile(bad, np.array([0, 1000, 2000], np.uint64))
    assert e.value.code == A.E_NON_ACGT
    # both outputs NULL; no sequence at all
    with pytest.raises(lib.KmuError) as e:
        c.read_profile(qb, qo, want_counts=False, want_stats=False)
    assert e.value.code == A.E_BAD_ARG
    gc, gs = c.read_profile(qb[:16], np.array([0], np.uint64))
    assert gs.size == 0
    # nothing but sequences shorter than k
    gs = c.read_profile(qb[:40], np.array([0, 0, 10, 40], np.uint64), want_counts=False)
    assert np.array_equal(gs, np.zeros(3, DT))
    c.close()


# ---- the mirrors ---------------------------------------------------------------------------------------------------------------
def test_mirrors(ctx, oracle, tmp_path):
    from kmerutils_amd import kmercount, parsefastq
    ab, ao, o, (qb, qo) = case(oracle, A.KMER64BIT, 31)
    kc = kmercount.KmerCounter(31, 1 << 16, 8, ctx=ctx)
    kc.insert_reads((ab, ao))
    assert np.array_equal(kc.get_count_histogram(), kc.raw.histogram())
    mc, ms = kc.get_reads_abundance((qb, qo), 3)
    rc, rs = kc.raw.read_profile(qb, qo, 3)
    assert np.array_equal(mc, rc) and np.array_equal(ms, rs)
    # parsefastq --histo: count<TAB>number of distinct k-mers, one line per non-empty bin, ascending
    fq = tmp_path / "tiny.fastq"
    with open(fq, "w") as f:
        for i in range(12):
            s = ab[int(ao[i]):int(ao[i + 1])].tobytes().decode()
            f.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
        f.write("@poly\n%s\n+\n%s\n" % ("A" * 400, "I" * 400))
    histo = tmp_path / "tiny.histo"
    assert parsefastq.main(["-f", str(fq), "-s", "31", "--outdir", str(tmp_path), "--histo", str(histo)]) == 0
    oc = oracle.Counter(A.KMER64BIT, 31, 16, 1 << 16)
    sub_b, sub_o = _cat([(ab[:int(ao[12])], ao[:13]), (np.frombuffer(b"A" * 400, np.uint8), np.array([0, 400], np.uint64))])
    oc.add_reads(sub_b, sub_o)
    want = np.bincount(np.minimum(oc.dump(1)[1], 255).astype(np.int64))
    lines = ["%d\t%d" % (v, want[v]) for v in np.flatnonzero(want)]
    assert open(histo).read().splitlines() == lines and lines[-1] == "255\t1"

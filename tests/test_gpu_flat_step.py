"""The flat-stream wave step (kmu_flat.h) under every kernel that is written on it, on one small read set whose read ends sit
where the step can go wrong: next to the 16-base word of a lane (15, 16, 17), next to the 1 024-base step of a wave (1023, 1024,
1025, 2047, 2048) and at the end of the stream (exactly 3 x 1024, and 5 bases past it).  Among the reads are lengths 0, 1, k - 1 and
k, and a run of 70 reads of fewer than 16 bases each: more read starts inside one step than the hinted search looks at.  A third
stream lets the last read run on to 6 x 1024: two steps lie wholly inside it (no per-k-mer boundary test), and a wave of the
one-block kernels takes a second step, so that the hinted search is used -- once past the run (it falls back), once inside the
last read.

Compared for equality with the oracle's counter, for (Kmer16b32bit, 16), (Kmer64bit, 21) and (Kmer64bit, 31) -- with k = 31 every
k-mer that starts at base 2 or later of a lane's word needs the third word of its window: add_reads + dump through direct insertion
(k_count_add_flat) and through the exact levels of the partitioned build (k_part_hist1, k_part_scatter1_exact), once_positions
(k_once_count, k_once_emit) and read_profile (k_count_profile); host and device input, and device ranges `offsets + first` whose
first read starts 1023, 1024 and 1040 bases into the stream."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A
from test_gpu_count_readback import dev, dev_stats, expected

pytestmark = pytest.mark.gpu

KMERS = [(A.KMER16B32BIT, 16), (A.KMER64BIT, 21), (A.KMER64BIT, 31)]
KMER_IDS = ["k16", "k21", "k31"]
TAILS = [0, 5, 3 * 1024]  # bases of the last read past flat position 3 x 1024
TAIL_IDS = ["ends_on_step", "five_past", "long_last_read"]
BITS = 8
RUN = 70  # reads of the run of short reads


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def read_lengths(tail):
    rng = np.random.default_rng(0xF1A7)
    lens = [15, 1, 1, 0]                                      # ends at 15, 16, 17; an empty read
    lens += [int(v) for v in rng.integers(1, 10, size=RUN)]   # the run: 70 reads inside step 0
    lens += [15, 16, 20, 21, 30, 31]                          # k - 1 and k
    lens += [1023 - sum(lens), 1, 1, 15]                      # ends at 1023, 1024, 1025, 1040
    lens += [2047 - sum(lens), 1]                             # ends at 2047, 2048
    lens += [1024 + tail]
    return lens


_READS, _WANT = {}, {}


def reads(oracle, tail):
    """(sequences, bases, offsets): ACGT only, slices of either strand of a circular genome of 3 000 bases, so that k-mers occur
    once, twice and more often"""
    if tail not in _READS:
        rng = np.random.default_rng(0x5EED)
        genome = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=3000).tobytes() * 3
        rc = bytes.maketrans(b"ACGT", b"TGCA")
        seqs = []
        for i, L in enumerate(read_lengths(tail)):
            s0 = int(rng.integers(0, 3000))
            s = genome[s0:s0 + L]
            seqs.append(s[::-1].translate(rc) if i % 2 else s)
        bases, off = oracle.concat(seqs)
        ends = set(int(v) for v in off[1:])
        assert {15, 16, 17, 1023, 1024, 1025, 1040, 2047, 2048} <= ends and int(off[-1]) == 3 * 1024 + tail
        assert int(off[4 + RUN]) < 1024 and (np.diff(off[4:5 + RUN].astype(np.int64)) < 16).all()
        _READS[tail] = (seqs, bases, off)
    return _READS[tail]


def want(oracle, tail, ktype, k):
    """what the oracle says of the whole read set: computed once per case, shared, never changed"""
    if (tail, ktype, k) not in _WANT:
        _, bases, off = reads(oracle, tail)
        o = oracle.Counter(ktype, k, BITS, 1 << 14)
        o.add_reads(bases, off)
        wk, wc = o.dump(1)
        once = o.once_positions(bases, off)
        cnt, st = expected(oracle, o, bases, off, ktype, k, BITS, 2)
        assert 0 < once[0].size < wc.sum() and wc.max() >= 2 and (st["n_kmers"] == 0).sum() > RUN and (st["n_kmers"] == 1).any()
        _WANT[(tail, ktype, k)] = dict(dump=(wk, wc), once=once, counts=cnt, stats=st)
    return _WANT[(tail, ktype, k)]


def first_at(off, pos):
    return int(np.flatnonzero(off == pos)[0])


def dump_of(ctx, ktype, k, bases, off):
    c = ctx.counter(ktype, k, BITS, 1 << 14)
    c.add_reads(bases, off)
    got = c.dump(1)
    c.close()
    return got


@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_dump_direct_and_partitioned(ctx, oracle, monkeypatch, ktype, k, tail):
    _, bases, off = reads(oracle, tail)
    wk, wc = want(oracle, tail, ktype, k)["dump"]
    for path in ("direct", "partitioned"):
        monkeypatch.setenv("KMU_COUNT_PATH", path)
        for b, o in ((bases, off), (dev(bases), dev(off))):
            gk, gc = dump_of(ctx, ktype, k, b, o)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc), path


@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_once_positions_and_read_profile(ctx, oracle, ktype, k, tail):
    _, bases, off = reads(oracle, tail)
    w = want(oracle, tail, ktype, k)
    c = ctx.counter(ktype, k, BITS, 1 << 14)
    c.add_reads(bases, off)
    for got in (c.once_positions(bases, off), [t.cpu().numpy() for t in c.once_positions(dev(bases), dev(off))]):
        for g, x in zip(got, w["once"]):
            assert np.array_equal(g.view(x.dtype), x)
    gc, gs = c.read_profile(bases, off)
    assert np.array_equal(gc, w["counts"]) and np.array_equal(gs, w["stats"])
    dc, ds = c.read_profile(dev(bases), dev(off))  # (positions that start no k-mer keep the zeros the array came with)
    assert np.array_equal(dc.cpu().numpy().view(np.uint16), w["counts"]) and np.array_equal(dev_stats(ds), w["stats"])
    c.close()


@pytest.mark.parametrize("tail", TAILS, ids=TAIL_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_device_ranges(ctx, oracle, monkeypatch, ktype, k, tail):
    """`offsets + first` of device-resident reads: the walk starts at the wave step that holds offsets[first] -- 1023 bases before
    the next step, on a step, and one word past a step (lane 0 of the step then lies before the range)"""
    import torch
    seqs, bases, off = reads(oracle, tail)
    w = want(oracle, tail, ktype, k)
    wk, ws, wp = w["once"]
    n = off.size - 1
    db, do = dev(bases), dev(off)
    whole = ctx.counter(ktype, k, BITS, 1 << 14)
    whole.add_reads(bases, off)
    for first, last in ((first_at(off, 1023), n), (first_at(off, 1024), first_at(off, 2048)), (first_at(off, 1040), n)):
        sub_b, sub_o = oracle.concat(seqs[first:last])
        o = oracle.Counter(ktype, k, BITS, 1 << 14)
        o.add_reads(sub_b, sub_o)
        sk, sc = o.dump(1)
        for path in ("direct", "partitioned"):
            monkeypatch.setenv("KMU_COUNT_PATH", path)
            gk, gc = dump_of(ctx, ktype, k, db, do[first:last + 1])
            assert np.array_equal(gk, sk) and np.array_equal(gc, sc), (first, last, path)
        monkeypatch.delenv("KMU_COUNT_PATH")
        # against the counter of the whole set; the records of a range are relative to the range
        rk, rs, rp = whole.once_positions(db, do[first:last + 1])
        sel = (ws >= first) & (ws < last)
        assert np.array_equal(rk.cpu().numpy().view(np.uint64), wk[sel])
        assert np.array_equal(rs.cpu().numpy().view(np.uint32), ws[sel] - first) and np.array_equal(rp.cpu().numpy().view(np.uint32), wp[sel])
        # counts at the caller's indices, nothing written outside the k-mer starts of the range
        sent = torch.full((int(off[-1]),), 0x5A5A, dtype=torch.int16, device="cuda")
        dc, dst = whole.read_profile(db, do[first:last + 1], counts_out=sent)
        wcnt = np.full(int(off[-1]), 0x5A5A, np.uint16)
        for i in range(first, last):
            b, m = int(off[i]), max(int(off[i + 1]) - int(off[i]) - k + 1, 0)
            wcnt[b:b + m] = w["counts"][b:b + m]
        assert np.array_equal(dc.cpu().numpy().view(np.uint16), wcnt), (first, last)
        assert np.array_equal(dev_stats(dst), w["stats"][first:last])
    whole.close()

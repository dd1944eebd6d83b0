"""k_multiset_long takes the reads of more than 20 480 places (place = position + the read's lead in its first staged word, offsets[r]
mod 16) that the two shapes of k_multiset_uq leave behind: a read of nk k-mers is cut into P = ceil(nk / T_P) sub-lists by key hash,
T_P = 16 384, and every sub-list goes through the uq step.  Its launch is timed under the general kernel's name, k_sketch_pmh3a, and so
is the launch of the general kernel for the reads it hands back: one launch under that name = nothing fell back, two = something did.
The rows must be the oracle's, bit for bit."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

K, M = 31, 200
T_P = 16384              # PMH_LONG_TP
UQ2_MAX = 20 * 1024      # places the second uq shape holds
LONG_SEQ_KMERS = 1 << 18  # the per-sequence route hands longer sequences to the all-sequences path
DEF_PARTS = 32
LEADS = (0, 1, 7, 15)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _params(k=K, m=M):
    return A.SketchParams(A.ALGO_PROB3A, A.KMER64BIT, k, m, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)


def _rnd(rng, n):
    return rng.choice(ACGT, size=int(n)).tobytes()


def _at_lead(rng, seqs, lead):
    """a filler read (40 .. 55 bases) so that the next read starts at `lead` mod 16"""
    at = sum(len(s) for s in seqs)
    seqs.append(_rnd(rng, 40 + (lead - (at + 40)) % 16))
    assert (at + len(seqs[-1])) % 16 == lead


def _run(oracle, monkeypatch, seqs, p):
    """the batch through the two-kernel route -> (rows, launches by timer name)"""
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_PMH_SPLIT", "1")  # the (key, weight) lists also for a small batch
    monkeypatch.delenv("KMU_PMH_PLAIN", raising=False)
    monkeypatch.delenv("KMU_PMH_SHORT", raising=False)
    bases, off = oracle.concat(seqs)
    ctx = lib.Context(0)
    try:
        ctx.profile_reset()
        ctx.profile_enable(True)
        got = np.asarray(ctx.sketch(bases, off, p))
        ctx.profile_enable(False)
        prof = ctx.profile_get()
    finally:
        ctx.close()
    return got, {n: v[0] for n, v in prof.items()}, bases, off


def _sketch(oracle, monkeypatch, seqs, p, uq_launches, general_launches):
    got, launches, bases, off = _run(oracle, monkeypatch, seqs, p)
    assert launches.get("k_multiset_uq", 0) == uq_launches, sorted(launches.items())
    assert launches.get("k_sketch_pmh3a", 0) == general_launches, sorted(launches.items())
    want = oracle.sketch(bases, off, p)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "rows differ from the oracle: reads %s (lengths %s, leads %s)" % (
        bad[:8].tolist(), [len(seqs[i]) for i in bad[:8]], [int(off[i]) % 16 for i in bad[:8]])
    return got, want


@pytest.mark.parametrize("m", (64, 200))
@pytest.mark.parametrize("k", (21, 31, 32))
def test_partition_edges(oracle, monkeypatch, k, m):
    """nk + lead at the first place beyond the second uq shape and around 2 T_P and 3 T_P, at leads 0, 1, 7 and 15 (nk itself then
    lies on both sides of every edge of P): two, three and four sub-lists, nothing falls back.
    k = 32 is not a k-mer size of Kmer64bit (check_kmer: at most 31 bases, as upstream, whose push mask is 0 at 32): no kernel of any
    route ever sees it, and the case holds the library to that refusal, on this batch as on any other."""
    from kmerutils_amd import lib
    rng = np.random.default_rng(4101 + k)
    spans = (UQ2_MAX + 1, 2 * T_P - 1, 2 * T_P, 2 * T_P + 1, 3 * T_P, 3 * T_P + 1)
    assert spans == (20481, 32767, 32768, 32769, 49152, 49153)
    seqs = []
    for lead in LEADS:
        for span in spans:
            _at_lead(rng, seqs, lead)
            seqs.append(_rnd(rng, span - lead + k - 1))
    if k == 32:
        with pytest.raises(lib.KmuError) as e:
            _run(oracle, monkeypatch, seqs, _params(k, m))
        assert e.value.code == A.E_BAD_K
        return
    _sketch(oracle, monkeypatch, seqs, _params(k, m), uq_launches=2, general_launches=1)


def _np_int64_hash(key):
    with np.errstate(over="ignore"):
        key = key.astype(np.uint64)
        key = ~key + (key << np.uint64(21))
        key = key ^ (key >> np.uint64(24))
        key = (key + (key << np.uint64(3))) + (key << np.uint64(8))
        key = key ^ (key >> np.uint64(14))
        key = (key + (key << np.uint64(2))) + (key << np.uint64(4))
        key = key ^ (key >> np.uint64(28))
        key = key + (key << np.uint64(31))
    return key


def _keys(seq, k=K):
    """int64_hash of the canonical k-mer at every position of the read (A, C, G, T = 0 .. 3, first base in the top bits)"""
    lut = np.zeros(256, np.uint64)
    lut[list(b"ACGT")] = np.arange(4, dtype=np.uint64)
    c = lut[np.frombuffer(seq, np.uint8)]
    n = len(seq) - k + 1
    val = np.zeros(n, np.uint64)
    rc = np.zeros(n, np.uint64)
    for j in range(k):
        val |= c[j:j + n] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return _np_int64_hash(np.minimum(val, rc))


def test_equal_keys_far_apart(oracle, monkeypatch):
    """a 1 500-base stretch copied 29 000 places downstream (another tile of the scan) and a 200-base one inserted as its reverse
    complement: ~ 1 640 keys of weight 2, ~ 550 per sub-list (1 100 collected keys beside ~ 550 that only share a bitmap bit: under
    UQ2_COLL = 2 048), found in a sub-list wherever their two places are.  What the comparison rests on is asserted first: slots of the
    oracle's row are held by keys of weight 2 (the row could not tell them from two entries of weight 1 else)"""
    rng = np.random.default_rng(4102)
    s = bytearray(_rnd(rng, 36000))
    s[30000:31500] = s[1000:2500]
    s[33000:33200] = bytes(s[4000:4200]).translate(COMP)[::-1]
    s = bytes(s)
    keys = _keys(s)
    uniq, cnt = np.unique(keys, return_counts=True)
    dup = uniq[cnt >= 2]
    assert 1600 <= dup.size <= 1680, dup.size
    p = _params()
    want = oracle.sketch(*oracle.concat([s]), p)
    assert np.isin(want[0], uniq).all(), "the row's entries are keys of the read"
    assert int(np.isin(want[0], dup).sum()) >= 4
    got, _ = _sketch(oracle, monkeypatch, [s], p, uq_launches=2, general_launches=1)
    assert np.array_equal(got[0], want[0])


def test_fall_back(oracle, monkeypatch):
    """a 25 kb homopolymer (one key: its sub-list outgrows the registers) and two copies of the same 15 kb (every key is in a collision
    group: more than a sub-list collects) go back to the general kernel: two launches under its name"""
    rng = np.random.default_rng(4103)
    half = _rnd(rng, 15000)
    _sketch(oracle, monkeypatch, [b"A" * 25000, half + half], _params(), uq_launches=2, general_launches=2)


def test_many_partitions(oracle, monkeypatch):
    """the longest read the per-sequence route keeps, LONG_SEQ_KMERS = 2^18 k-mers: 16 sub-lists.  A read of DEF_PARTS + 1 = 33 sub-lists
    (more than 32 x 16 384 = 524 288 k-mers) never reaches the kernel: a batch with a sequence of more than 2^18 k-mers does not take the
    lists at all (pmh_route: skip_longer), its long sequence goes through the all-sequences path -- the second batch below, which
    only has to give the oracle's rows."""
    rng = np.random.default_rng(4104)
    assert -(-LONG_SEQ_KMERS // T_P) == 16 <= DEF_PARTS
    _sketch(oracle, monkeypatch, [_rnd(rng, 3000), _rnd(rng, LONG_SEQ_KMERS + K - 1)], _params(), uq_launches=2, general_launches=1)
    seqs = [_rnd(rng, 25000), _rnd(rng, DEF_PARTS * T_P + 1 + K - 1)]
    got, launches, bases, off = _run(oracle, monkeypatch, seqs, _params())
    assert launches.get("k_multiset_uq", 0) == 0, sorted(launches.items())
    assert np.array_equal(got, oracle.sketch(bases, off, _params()))


@pytest.mark.parametrize("k,m", ((31, 200), (21, 64)), ids=("k31_m200", "k21_m64"))
def test_mixed_queue_in_both_orders(oracle, monkeypatch, k, m):
    """reads for every stage interleaved -- first shape, second shape, this kernel (two to four sub-lists), a read that falls back --
    and reads of k and k - 1 bases between them; and the same batch in reversed order"""
    rng = np.random.default_rng(4105)
    half = _rnd(rng, 12000)
    seqs = []
    for n in (25000, 300, 9000, 44000, 15000, 21000, 60, 30000, 5000, 58000, 19000, 23000):
        seqs.append(_rnd(rng, n))
        seqs.append(_rnd(rng, k))
        seqs.append(_rnd(rng, k - 1))
    seqs.insert(7, half + half)
    seqs.insert(20, b"AC" * 11000)
    p = _params(k, m)
    fwd, _ = _sketch(oracle, monkeypatch, seqs, p, uq_launches=2, general_launches=2)
    rev, _ = _sketch(oracle, monkeypatch, seqs[::-1], p, uq_launches=2, general_launches=2)
    assert np.array_equal(fwd, rev[::-1])


def test_n_in_the_second_tile(oracle, monkeypatch):
    """an N at place 25 000 of a read of 30 000 bases (the scan's second tile): the call fails with the non-ACGT error, as it did when
    the general kernel took the read"""
    from kmerutils_amd import lib
    rng = np.random.default_rng(4106)
    s = bytearray(_rnd(rng, 30000))
    s[25000] = ord("N")
    with pytest.raises(lib.KmuError) as e:
        _run(oracle, monkeypatch, [_rnd(rng, 5000), bytes(s), _rnd(rng, 26000)], _params())
    assert e.value.code == A.E_NON_ACGT

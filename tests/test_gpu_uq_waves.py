"""A wave of k_multiset_uq owns 256 consecutive places of a group of four register slots -- group g of thread t stands for places
4 (t + T g) .. + 3 (place = position + the read's lead in its first staged word, offsets[r] mod 16; T = 512 / 1 024 threads) -- and a
read ends inside one wave: the waves behind that one skip the group, in the key phase and in the sort-out phase, by one scalar test,
and their slots hold whatever an earlier read left there.  The rows must be the oracle's, bit for bit: at every wave edge and lead,
for equal k-mers on both sides of a wave edge, for short reads between full ones, and in both read orders.  (Phase B of
k_multiset_long -- slot q of thread t = entry 1 024 q + t of a sub-list -- skips whole groups only: the same test per wave bought
nothing there, DESIGN 7.  Its sub-lists that end at a wave edge are held here all the same.)"""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

M = 200
WAVE = 256                          # places of a group a wave owns
G1, G2 = 4 * 512, 4 * 1024          # places per group: first / second shape
UQ1_MAX, UQ2_MAX = 5 * G1, 5 * G2   # places the shapes hold
T_P = 16384                         # PMH_LONG_TP: keys a sub-list of k_multiset_long expects at most
LEADS = (0, 1, 15)
KS = (31, 21)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _params(k, m=M):
    return A.SketchParams(A.ALGO_PROB3A, A.KMER64BIT, k, m, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)


def _rnd(rng, n):
    return rng.choice(ACGT, size=int(n)).tobytes()


class _Batch:
    """reads appended one behind the other; a short filler read in front of a read puts it at the lead asked for"""

    def __init__(self, rng, k):
        self.rng, self.k, self.seqs, self.at = rng, k, [], 0

    def add(self, s):
        self.seqs.append(bytes(s))
        self.at += len(s)
        return len(self.seqs) - 1

    def at_lead(self, lead):
        self.add(_rnd(self.rng, 40 + (lead - (self.at + 40)) % 16))
        assert self.at % 16 == lead

    def add_span(self, span, lead):
        """a random read whose k-mers plus lead are exactly `span` places"""
        assert span - lead >= 1
        self.at_lead(lead)
        return self.add(_rnd(self.rng, span - lead + self.k - 1))


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
    return got, {n: v[0] for n, v in prof.items()}, off


def _both_orders(oracle, monkeypatch, seqs, p, uq, pmh3a):
    """the batch as it stands and reversed (every read then stands at another lead) against the oracle's rows, computed once; the
    launches under k_multiset_uq's name and under k_sketch_pmh3a's (k_multiset_long's launch, and one more for what it hands back)"""
    want = oracle.sketch(*oracle.concat(seqs), p)
    for order, w in ((seqs, want), (seqs[::-1], want[::-1])):
        got, launches, off = _run(oracle, monkeypatch, order, p)
        assert launches.get("k_multiset_uq", 0) == uq, sorted(launches.items())
        assert launches.get("k_sketch_pmh3a", 0) == pmh3a, sorted(launches.items())
        bad = np.nonzero((got != w).any(axis=1))[0]
        assert bad.size == 0, "rows differ from the oracle: reads %s (lengths %s, leads %s)" % (
            bad[:8].tolist(), [len(order[i]) for i in bad[:8]], [int(off[i]) % 16 for i in bad[:8]])
    return want


@pytest.mark.parametrize("k", KS)
def test_wave_edges_first_shape(oracle, monkeypatch, k):
    """spans one under, at and one over 256 w: inside the first group, across the first group edge (2 048) and at the last wave of the
    last group (10 240; 10 241 is the second shape's first read), at leads 0, 1 and 15"""
    b = _Batch(np.random.default_rng(5101 + k), k)
    for lead in LEADS:
        for w in (1, 2, 7, 8, 9, 16, 39, 40):
            for span in (WAVE * w - 1, WAVE * w, WAVE * w + 1):
                b.add_span(span, lead)
    _both_orders(oracle, monkeypatch, b.seqs, _params(k), uq=2, pmh3a=0)


@pytest.mark.parametrize("k", KS)
def test_wave_edges_second_shape(oracle, monkeypatch, k):
    """the same for reads of 10 241 .. 20 480 places; 20 481 is k_multiset_long's first read"""
    b = _Batch(np.random.default_rng(5102 + k), k)
    for lead in LEADS:
        for w in (41, 48, 56, 64, 79, 80):
            for span in (WAVE * w - 1, WAVE * w, WAVE * w + 1):
                b.add_span(span, lead)
    _both_orders(oracle, monkeypatch, b.seqs, _params(k), uq=2, pmh3a=1)


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


def _keys(seq, k):
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


def _differ(s, i, j):
    """base j of the read is made another than base i (where both exist)"""
    if 0 <= i and j < len(s) and s[j] == s[i]:
        s[j] = b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]


def _planted(rng, k, span, lead, pairs):
    """a random read of `span` places at `lead` in which the k-mer at place a stands again at place b, for every (a, b) of `pairs`"""
    s = bytearray(_rnd(rng, span - lead + k - 1))
    for a, b in pairs:
        pa, pb = a - lead, b - lead
        assert 0 <= pa and pa + k <= pb and pb + k <= len(s)
        s[pb:pb + k] = s[pa:pa + k]
        _differ(s, pa - 1, pb - 1)  # (the copy ends where it ends: the bases on either side of it are not the source's)
        _differ(s, pa + k, pb + k)
    s = bytes(s)
    _, cnt = np.unique(_keys(s, k), return_counts=True)
    assert sorted(cnt[cnt > 1].tolist()) == [2] * len(pairs), "the planted k-mers and no others occur twice"
    return s


@pytest.mark.parametrize("k", KS)
def test_equal_kmers_across_a_wave_edge(oracle, monkeypatch, k):
    """reads that end inside wave 3 of a group (77 places of it): a k-mer of that last, partly filled wave equals one of wave 0 of the
    same group, another one equals a k-mer of an earlier group; and a read whose only equal k-mers both stand in that last wave.
    These are the keys the collision sort must still merge: the row's slots would else hold them at weight 1."""
    rng = np.random.default_rng(5103 + k)
    b = _Batch(rng, k)
    for grp, g in ((G1, 1), (G1, 4), (G2, 3), (G2, 4)):  # (places per group, the group the read ends in)
        first = grp * g  # first place of that group; its wave 3: first + 768 .. first + 844
        span = first + 3 * WAVE + 77
        for lead in LEADS:
            b.at_lead(lead)
            b.add(_planted(rng, k, span, lead, ((first + 100, first + 3 * WAVE + 5), (500, first + 3 * WAVE + 45))))
            b.at_lead(lead)
            b.add(_planted(rng, k, span, lead, ((first + 3 * WAVE + 2, first + 3 * WAVE + 44),)))
    _both_orders(oracle, monkeypatch, b.seqs, _params(k), uq=2, pmh3a=0)


@pytest.mark.parametrize("k", KS)
def test_short_reads_between_full_ones(oracle, monkeypatch, k):
    """a read of one wave's worth of k-mers directly behind a full-length read and in front of one, for both shapes: the slots its
    idle waves skip carry the last read's keys.  A read of k - 1 bases between such reads has a row of zeros.
    (Full-length: the shape's places less 16 k-mers -- at whatever lead the read stands, in either order, its last wave of the last
    group has k-mers and the read stays the shape's.)"""
    rng = np.random.default_rng(5104 + k)
    b = _Batch(rng, k)
    no_key = []
    for full in (UQ1_MAX, UQ2_MAX):
        for short in (1, 200, WAVE, WAVE + 1):
            b.add(_rnd(rng, full - 16 + k - 1))
            b.add(_rnd(rng, short + k - 1))
            b.add(_rnd(rng, full - 16 + k - 1))
            no_key.append(b.add(_rnd(rng, k - 1)))
            b.add(_rnd(rng, 130 + k - 1))
    b.add(_rnd(rng, UQ1_MAX - 16 + k - 1))
    want = _both_orders(oracle, monkeypatch, b.seqs, _params(k), uq=2, pmh3a=0)
    assert not want[no_key].any()


@pytest.mark.parametrize("what", ("empty", "N"))
def test_errors_between_full_reads(oracle, monkeypatch, what):
    """an empty read, and a short read with an N, between full-length reads: the call's error code, in both orders"""
    from kmerutils_amd import lib
    k = 31
    rng = np.random.default_rng(5105)
    b = _Batch(rng, k)
    b.add_span(UQ1_MAX, 0)
    b.add(b"" if what == "empty" else _rnd(rng, 100) + b"N" + _rnd(rng, 100))
    b.add_span(UQ1_MAX - 300, 1)
    b.add(_rnd(rng, 150))
    b.add_span(UQ2_MAX, 15)
    for seqs in (b.seqs, b.seqs[::-1]):
        with pytest.raises(lib.KmuError) as e:
            _run(oracle, monkeypatch, seqs, _params(k))
        assert e.value.code == (A.E_EMPTY_SEQ if what == "empty" else A.E_NON_ACGT)


def _part_of(keys, parts):
    """pmh_long_part_of"""
    with np.errstate(over="ignore"):
        lo, hi = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32)
        z = (lo + hi * np.uint32(0x9E3779B9)) * np.uint32(0xC2B2AE3D)
    return ((z.astype(np.uint64) * np.uint64(parts)) >> np.uint64(32)).astype(np.int64)


@pytest.mark.parametrize("k", KS)
def test_sub_lists_of_the_long_kernel(oracle, monkeypatch, k):
    """k_multiset_long: a read of about 40 000 k-mers (three sub-lists of ~ 13 300 keys: each ends inside its fourth group); a read cut
    so that one of its three sub-lists holds 12 288 + 64 j keys, j in 1 .. 15 (the fourth group's first slot ends exactly at a wave
    edge: the waves behind it have no entry in that group); a 25 kb homopolymer the kernel hands back to the general one (a second
    launch under that kernel's name); short reads between them"""
    rng = np.random.default_rng(5106 + k)
    s = _rnd(rng, 40000 + k - 1)
    part = _part_of(_keys(s, k), 3)
    cut = None
    for nk in range(3 * 12288 + 64, 3 * 13312):  # (P = 3 for every prefix here)
        cnt = np.bincount(part[:nk], minlength=3)
        hit = (cnt > 12288) & (cnt < 13312) & (cnt % 64 == 0)
        if hit.any():
            cut = nk
            break
    assert cut is not None and -(-cut // T_P) == 3
    seqs = [s, _rnd(rng, 300), s[:cut + k - 1], _rnd(rng, 9000), b"A" * 25000, _rnd(rng, 60)]
    _both_orders(oracle, monkeypatch, seqs, _params(k), uq=2, pmh3a=2)

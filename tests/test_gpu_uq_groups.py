"""k_multiset_uq works its twenty register slots per thread in five groups of four; group g of a workgroup stands for places
[4 T g, 4 T (g + 1)) of the read (place = position + the read's lead in its first staged word, offsets[r] mod 16; T = 512 threads
in the first shape, 1 024 in the second).  Both phases of the kernel skip the groups a read does not reach, by one uniform test,
and the slots of a skipped group hold no key of this read: whatever an earlier read of the workgroup left in the registers.  The rows must be the oracle's, bit for
bit: at every group edge and every lead, for equal k-mers on both sides of an edge, and for short reads behind long ones."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

K, M = 31, 200
G1, G2 = 4 * 512, 4 * 1024       # places per group: first / second shape
UQ1_MAX, UQ2_MAX = 5 * G1, 5 * G2  # places the shapes hold
LEADS = (0, 1, 7, 15)
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def _params(k=K, m=M):
    return A.SketchParams(A.ALGO_PROB3A, A.KMER64BIT, k, m, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)


def _rnd(rng, n):
    return rng.choice(ACGT, size=int(n)).tobytes()


class _Batch:
    """reads appended one behind the other; a short filler read in front of a read puts it at the lead asked for"""

    def __init__(self, rng, k=K):
        self.rng, self.k, self.seqs, self.at = rng, k, [], 0

    def add(self, s):
        self.seqs.append(bytes(s))
        self.at += len(s)
        return len(self.seqs) - 1

    def at_lead(self, lead):
        """a filler read (40 .. 55 bases: a handful of k-mers of its own) so that the next read starts at `lead` mod 16"""
        self.add(_rnd(self.rng, 40 + (lead - (self.at + 40)) % 16))
        assert self.at % 16 == lead

    def add_span(self, span, lead):
        """a random read whose k-mers plus lead are exactly `span` places"""
        assert span - lead >= 1
        self.at_lead(lead)
        return self.add(_rnd(self.rng, span - lead + self.k - 1))


def _sketch(oracle, monkeypatch, seqs, p, uq_launches, general=None):
    """the batch through the two-kernel route -> rows, checked against the oracle; k_multiset_uq launched `uq_launches` times"""
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
    assert prof.get("k_multiset_uq", (0, 0.0))[0] == uq_launches, sorted((n, v[0]) for n, v in prof.items())
    if general is not None:
        assert (prof.get("k_sketch_pmh3a", (0, 0.0))[0] > 0) == general, sorted((n, v[0]) for n, v in prof.items())
    want = oracle.sketch(bases, off, p)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "rows differ from the oracle: reads %s (lengths %s, leads %s)" % (
        bad[:8].tolist(), [len(seqs[i]) for i in bad[:8]], [int(off[i]) % 16 for i in bad[:8]])
    return got


def test_group_edges_first_shape(oracle, monkeypatch):
    """nk + lead at, one under and one over every group edge of the first shape, at leads 0, 1, 7 and 15.  (nk + lead = 1 exists at
    lead 0 alone -- a read of the kernel's has a k-mer; the other leads take their smallest span, lead + 1, in its place.)"""
    b = _Batch(np.random.default_rng(3101))
    spans = (1, G1 - 1, G1, G1 + 1, 2 * G1, 2 * G1 + 1, 3 * G1, 4 * G1, UQ1_MAX - 1, UQ1_MAX)
    assert spans == (1, 2047, 2048, 2049, 4096, 4097, 6144, 8192, 10239, 10240)
    for lead in LEADS:
        for span in spans:
            b.add_span(max(span, lead + 1), lead)
    _sketch(oracle, monkeypatch, b.seqs, _params(), uq_launches=1, general=False)


def test_group_edges_second_shape(oracle, monkeypatch):
    """the reads the first shape hands on: the second shape's edges (groups of 4 096 places), and 20 481 places: the general kernel's"""
    b = _Batch(np.random.default_rng(3102))
    spans = (UQ1_MAX + 1, 3 * G2, 3 * G2 + 1, 4 * G2, 4 * G2 + 1, UQ2_MAX - 1, UQ2_MAX)
    assert spans == (10241, 12288, 12289, 16384, 16385, 20479, 20480)
    for lead in LEADS:
        for span in spans:
            b.add_span(span, lead)
    _sketch(oracle, monkeypatch, b.seqs, _params(), uq_launches=2, general=False)
    b.add_span(UQ2_MAX + 1, 0)
    b.add_span(UQ2_MAX + 1, 15)
    _sketch(oracle, monkeypatch, b.seqs, _params(), uq_launches=2, general=True)


def _plant_pair(rng, n, lead, place_a, place_b, revcomp, k=K):
    """a random read of n bases at `lead` in which the k-mer at place_a occurs again (itself, or its reverse complement) at place_b"""
    s = bytearray(_rnd(rng, n))
    pa, pb = place_a - lead, place_b - lead
    assert 0 <= pa < pb and pb + k <= n
    d = pb - pa
    if not revcomp:
        for i in range(pa + d, pb + k):  # (d < k: a stretch of period d; else a plain copy)
            s[i] = s[i - d]
        assert s[pa:pa + k] == s[pb:pb + k]
    else:
        assert d >= k or d % 2 == 1  # (overlapping: no base may be its own complement's partner)
        for i in range(k):           # s[pb + i] = complement of s[pa + k - 1 - i]
            lo, hi = sorted((pa + k - 1 - i, pb + i))
            s[hi] = COMP[s[lo]]
        assert bytes(COMP[c] for c in reversed(s[pa:pa + k])) == bytes(s[pb:pb + k])
    return bytes(s)


@pytest.mark.parametrize("revcomp", (False, True), ids=("same_strand", "reverse_complement"))
def test_equal_kmers_on_both_sides_of_a_group_edge(oracle, monkeypatch, revcomp):
    """a 31-mer (or its reverse complement) once in the last ten places of group g and once in the first ten of group g + 1, for every
    edge of both shapes, and once in group 0 and once in group 4: two register slots of different groups, one key of weight 2"""
    rng = np.random.default_rng(3103 + revcomp)
    b = _Batch(rng)
    planted = []
    for grp, cap, leads in ((G1, UQ1_MAX, LEADS), (G2, UQ2_MAX, (0, 7))):
        for lead in leads:
            for g in range(4):
                edge = grp * (g + 1)
                back, fwd = int(rng.integers(1, 11)), int(rng.integers(0, 10))
                if (back + fwd) % 2 == 0:  # an odd distance (see _plant_pair)
                    back = back - 1 if back > 1 else back + 1
                places = min(cap - lead, edge + int(rng.integers(100, grp - 100)))
                if grp == G2:
                    places = max(places, UQ1_MAX + 1)  # (the second shape's read)
                n = places - lead + K - 1
                b.at_lead(lead)
                planted.append(b.add(_plant_pair(rng, n, lead, edge - back, edge + fwd, revcomp)))
            b.at_lead(lead)  # groups 0 and 4
            planted.append(b.add(_plant_pair(rng, cap - lead + K - 1, lead, 100 + lead, 4 * grp + 100 + lead, revcomp)))
    got = _sketch(oracle, monkeypatch, b.seqs, _params(), uq_launches=2, general=False)
    # (what the comparison above rests on: the oracle counts the planted k-mer twice)
    for i in planted[:3]:
        cnt = oracle.Counter(A.KMER64BIT, K, 16, 1 << 17)
        cnt.add_reads(*oracle.concat([b.seqs[i]]))
        assert cnt.nb_distinct() < len(b.seqs[i]) - K + 1
    assert got.shape == (len(b.seqs), M)


MIXED = ((40, 60), (300, 60), (2100, 40), (9000, 30), (15000, 12), (30000, 4))  # (length, reads)


def _mixed(rng):
    lens = np.repeat([n for n, _ in MIXED], [c for _, c in MIXED])
    lens = lens[rng.permutation(len(lens))]
    # a workgroup takes four consecutive reads of the queue: a long read directly in front of a short one inside such a chunk
    # is what leaves stale keys in the slots the short read skips
    stale = sum(1 for i in range(len(lens) - 1) if i % 4 != 3 and lens[i] >= 9000 and lens[i + 1] <= 300)
    assert stale >= 5, stale
    return [_rnd(rng, n) for n in lens]


@pytest.mark.parametrize("k,m", ((31, 200), (21, 200), (31, 64)), ids=("k31_m200", "k21_m200", "k31_m64"))
def test_mixed_queue_in_both_orders(oracle, monkeypatch, k, m):
    """lengths 40 ... 30 000 interleaved: a thread's slots carry a long read's keys into a short read's turn; and the same batch
    in reversed order"""
    seqs = _mixed(np.random.default_rng(3105))
    p = _params(k, m)
    fwd = _sketch(oracle, monkeypatch, seqs, p, uq_launches=2, general=True)
    rev = _sketch(oracle, monkeypatch, seqs[::-1], p, uq_launches=2, general=True)
    assert np.array_equal(fwd, rev[::-1])


def test_reads_of_k_and_k_minus_one_bases_between_long_ones(oracle, monkeypatch):
    rng = np.random.default_rng(3106)
    seqs, one_key, no_key = [], [], []
    for n_long in (9000, 10000, 15000, 9500, 18000, 5000):
        seqs.append(_rnd(rng, n_long))
        one_key.append(len(seqs))
        seqs.append(_rnd(rng, K))
        seqs.append(_rnd(rng, n_long - 7))
        no_key.append(len(seqs))
        seqs.append(_rnd(rng, K - 1))
    seqs.append(_rnd(rng, 9000))
    got = _sketch(oracle, monkeypatch, seqs, _params(), uq_launches=2, general=False)
    assert not got[no_key].any(), "a read without a k-mer has a row of zeros"
    for r in one_key:  # every slot's point comes from the read's one key
        assert got[r].all() and np.unique(got[r]).size == 1, got[r][:4]

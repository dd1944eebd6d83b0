"""The key phases of k_multiset_uq and k_multiset_long send the four bitmap atomics of a slot group off together -- a slot without a key
ORs nothing into a word of its thread's own -- and look at the four answers afterwards; phase A of k_multiset_long does the same with
the four sub-list counters of a quarter; the next read's 16-byte chunks are requested in front of the key phase by an instruction the
compiler does not count and are waited for once, behind it.  What can go wrong is a lane without a key that disturbs the bitmap, an
answer taken for another slot's, and a chunk read before it has landed or landing on the wrong read.  The rows must be the oracle's,
bit for bit, with every batch sketched in both orders (place = position + the read's lead in its first staged word, offsets[r] mod 16;
a workgroup takes four consecutive reads of the queue and prefetches each from the turn of the one before)."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

K, M = 31, 200
UQ1_MAX, UQ2_MAX = 20 * 512, 20 * 1024  # places the two shapes hold
T_P = 16384                             # keys a sub-list of k_multiset_long expects at most
ACGT = np.frombuffer(b"ACGT", np.uint8)


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
        """a filler read (40 .. 55 bases) so that the next read starts at `lead` mod 16"""
        self.add(_rnd(self.rng, 40 + (lead - (self.at + 40)) % 16))
        assert self.at % 16 == lead

    def add_span(self, span, lead):
        """a random read whose k-mers plus lead are exactly `span` places"""
        assert span - lead >= 1
        self.at_lead(lead)
        return self.add(_rnd(self.rng, span - lead + self.k - 1))


def _run(oracle, monkeypatch, seqs, p):
    """the batch through the list route -> (rows, launches by timer name)"""
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_PMH_SPLIT", "1")  # the (key, weight) lists also for a small batch
    monkeypatch.delenv("KMU_PMH_PLAIN", raising=False)
    monkeypatch.setenv("KMU_PMH_SHORT", "0")  # ... through k_multiset_uq also where the longest read has at most 256 k-mers
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
    return got, {n: v[0] for n, v in prof.items()}


def _both_orders(oracle, monkeypatch, seqs, p, uq, pmh3a, pmh3a_reversed=-1):
    """the batch as it stands and reversed (other leads, every read behind the one it stood in front of) against the oracle's rows of
    the reads, computed once: a row depends on its read alone.  uq / pmh3a: launches under the timers k_multiset_uq and k_sketch_pmh3a
    (the latter is k_multiset_long's launch and, one more, the general kernel's for what is handed back); pmh3a_reversed: the same for
    the reversed batch where the other leads change it, None = whatever the leads make of it."""
    want = oracle.sketch(*oracle.concat(seqs), p)
    for order, name, n3a in ((seqs, "forward", pmh3a), (seqs[::-1], "reversed", pmh3a if pmh3a_reversed == -1 else pmh3a_reversed)):
        got, launches = _run(oracle, monkeypatch, order, p)
        assert launches.get("k_multiset_uq", 0) == uq, (name, sorted(launches.items()))
        assert n3a is None or launches.get("k_sketch_pmh3a", 0) == n3a, (name, sorted(launches.items()))
        if order is not seqs:
            got = got[::-1]
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert bad.size == 0, "%s: rows differ from the oracle: reads %s (lengths %s)" % (name, bad[:8].tolist(), [len(seqs[i]) for i in bad[:8]])
    return want


def first_shape_edges(edge):
    b = _Batch(np.random.default_rng(5100 + edge))
    for lead in range(16):
        for span in (edge - 1, edge, edge + 1):
            b.add_span(max(span, lead + 1), lead)  # (a read of the kernel's has a k-mer: nk + lead > lead)
        if edge == 4:
            for nk in (1, 2):
                b.at_lead(lead)
                b.add(_rnd(b.rng, nk + K - 1))
    return b.seqs


@pytest.mark.parametrize("edge", (4, 256, 2048, 4096, 10240))
def test_edges_of_the_first_shape(oracle, monkeypatch, edge):
    """nk + lead one under, at and one over a quarter (4 places), a wave (256), the first two slot groups (2 048, 4 096) and the shape
    (10 240: one over is the second shape's read), at every lead 0 .. 15; with the quarter, reads of exactly one and two k-mers"""
    seqs = first_shape_edges(edge)
    over = edge == UQ1_MAX
    _both_orders(oracle, monkeypatch, seqs, _params(), uq=2 if over else 1, pmh3a=0)


def second_shape_edges():
    b = _Batch(np.random.default_rng(5200))
    spans = (UQ1_MAX + 1, 3 * 4096 - 1, 3 * 4096, 3 * 4096 + 1, 4 * 4096 - 1, 4 * 4096, 4 * 4096 + 1, UQ2_MAX - 1, UQ2_MAX)
    assert spans == (10241, 12287, 12288, 12289, 16383, 16384, 16385, 20479, 20480)
    for lead in (0, 1, 7, 15):
        for span in spans:
            b.add_span(span, lead)
    return b.seqs


def test_edges_of_the_second_shape(oracle, monkeypatch):
    """reads of 10 241 .. 20 480 places: the first the second shape takes, its slot-group edges 4 096 g and its last.  (Reversed, a read
    of 20 480 k-mers stands at another lead and may be k_multiset_long's.)"""
    _both_orders(oracle, monkeypatch, second_shape_edges(), _params(), uq=2, pmh3a=0, pmh3a_reversed=None)


def repeats_beside_random_reads():
    rng = np.random.default_rng(5300)
    seqs = [_rnd(rng, UQ1_MAX - 15)]
    for n in (31, 34, 300, 5000):
        for unit in (b"A", b"AC"):
            seqs.append((unit * n)[:n])
            seqs.append(_rnd(rng, UQ1_MAX - 15))  # (at most 10 240 places at any lead)
    return seqs


def test_lanes_without_a_key_beside_contended_bits(oracle, monkeypatch):
    """homopolymers and reads of period two (one and two canonical 31-mers) of 31, 34, 300 and 5 000 bases: every key of a wave on one or
    two bits of the bitmap, beside lanes that have none; each directly behind and in front of a random read that fills the shape.
    5 000 bases are 4 970 keys in collision groups, more than either shape collects: back through the general kernel."""
    _both_orders(oracle, monkeypatch, repeats_beside_random_reads(), _params(), uq=2, pmh3a=2)


def one_kmer_reads_between_full_ones():
    rng = np.random.default_rng(5400)
    seqs = []
    for i in range(6):
        seqs.append(_rnd(rng, UQ1_MAX - 15))
        seqs.append(_rnd(rng, K))            # one k-mer
        seqs.append(_rnd(rng, (K - 1, 5, 1)[i % 3]))  # no k-mer: nothing to prefetch, a row of zeros
    return seqs + [_rnd(rng, UQ1_MAX - 15), _rnd(rng, K)]


def test_prefetch_between_one_kmer_and_full_reads(oracle, monkeypatch):
    """three chunk requests per thread behind one per workgroup and the other way round, reads shorter than k between them"""
    seqs = one_kmer_reads_between_full_ones()
    want = _both_orders(oracle, monkeypatch, seqs, _params(), uq=1, pmh3a=0)
    assert all(want[i].any() == (len(s) >= K) for i, s in enumerate(seqs))


def test_prefetch_batch_of_one_read(oracle, monkeypatch):
    """nothing to prefetch, nothing prefetched"""
    rng = np.random.default_rng(5401)
    for n in (K, 3000):
        _both_orders(oracle, monkeypatch, [_rnd(rng, n)], _params(), uq=1, pmh3a=0)


@pytest.mark.parametrize("tail", (1, 7, 15))
def test_prefetch_last_read_ends_with_the_buffer(oracle, monkeypatch, tail):
    """the last read ends where the base buffer ends, `tail` bytes into a 16-byte chunk: that chunk is not a whole one inside the array and
    is loaded bytewise behind the key phase instead of being requested ahead.  The read is the second and the third of its workgroup's
    four (prefetched from the turn of the read before it), and the only one of its batch"""
    rng = np.random.default_rng(5402 + tail)
    for n_front in (1, 6, 0):
        seqs = [_rnd(rng, 700 + 16 * i) for i in range(n_front)]
        at = sum(len(s) for s in seqs)
        seqs.append(_rnd(rng, 4000 + (tail - (at + 4000)) % 16))
        assert sum(len(s) for s in seqs) % 16 == tail
        _both_orders(oracle, monkeypatch, seqs, _params(), uq=1, pmh3a=0)


def test_prefetch_non_acgt_byte_in_a_chunk_requested_ahead(oracle, monkeypatch):
    """an N in a read that is prefetched from the turn of the read in front of it: the call fails with the non-ACGT error"""
    from kmerutils_amd import lib
    rng = np.random.default_rng(5403)
    for where in (0, 2999, 5999):
        s = bytearray(_rnd(rng, 6000))
        s[where] = ord("N")
        with pytest.raises(lib.KmuError) as e:
            _run(oracle, monkeypatch, [_rnd(rng, 5000), bytes(s), _rnd(rng, 700)], _params())
        assert e.value.code == A.E_NON_ACGT


def long_route_batch():
    rng = np.random.default_rng(5500)
    seqs = []
    for nk, short in ((UQ2_MAX + 1, 300), (2 * T_P + 1, K), (60000, 9000)):
        seqs.append(_rnd(rng, nk + K - 1))
        seqs.append(_rnd(rng, short))
    seqs.insert(3, b"AC" * 11000)  # two keys: one sub-list outgrows the registers -> the general kernel
    seqs.append(_rnd(rng, 15000))
    return seqs


def test_long_route(oracle, monkeypatch):
    """reads of 20 481 (the first k_multiset_long takes), 32 769 (three sub-lists) and 60 000 k-mers, a periodic read of 22 000 bases whose
    two keys overflow one sub-list (handed back to the general kernel), short reads and a second-shape read between them"""
    _both_orders(oracle, monkeypatch, long_route_batch(), _params(), uq=2, pmh3a=2)

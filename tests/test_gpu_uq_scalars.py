"""k_multiset_uq and k_multiset_long fetch the arguments they look at once per read or less -- the error word, the redo list, lst_n /
lst_nu / lst_w, the queue counters, read_list -- from the kernarg segment where they use them, form the k-mer mask and shift in front of
the key phase of every read, and address the two list counters from the lane.  Every path on which such an argument now arrives
differently is taken here by the smallest read that reaches it: no k-mer (lst_n = 0), an empty read and a non-ACGT byte (the error
word), the last read a shape holds and the first it hands on (redo_list and its counter, read_list in the next launch), a read whose
collision groups outgrow every shape (handed on three times), each with a short read directly behind it (the next-read and after-next
bookkeeping).  Rows are the oracle's bit for bit, every batch in both read orders, the reads in question at leads 0, 1 and 15."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

K, M = 31, 200
UQ1_MAX, UQ2_MAX = 20 * 512, 20 * 1024  # places (k-mers + the lead of the read's first base in its 16-byte chunk) the two shapes hold
LEADS = (0, 1, 15)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _params():
    return A.SketchParams(A.ALGO_PROB3A, A.KMER64BIT, K, M, A.SIG_U64, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)


def _rnd(rng, n):
    return rng.choice(ACGT, size=int(n)).tobytes()


class _Batch:
    """reads appended one behind the other; a filler read in front of a read puts it at the lead asked for"""

    def __init__(self, seed):
        self.rng, self.seqs, self.at = np.random.default_rng(seed), [], 0

    def add(self, s):
        self.seqs.append(bytes(s))
        self.at += len(s)
        return len(self.seqs) - 1

    def at_lead(self, lead):
        """a short filler read (40 .. 55 bases) so that the next read starts at `lead` mod 16: also the short read behind the last one"""
        self.add(_rnd(self.rng, 40 + (lead - (self.at + 40)) % 16))
        assert self.at % 16 == lead

    def add_span(self, span, lead):
        """a random read whose k-mers plus lead are exactly `span` places"""
        self.at_lead(lead)
        return self.add(_rnd(self.rng, span - lead + K - 1))

    def short(self):
        return self.add(_rnd(self.rng, 300))


def _run(oracle, monkeypatch, seqs):
    """the batch through the list route, the way tests/test_gpu_uq_overlap.py forces it -> (rows, launches by timer name)"""
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_PMH_SPLIT", "1")
    monkeypatch.delenv("KMU_PMH_PLAIN", raising=False)
    monkeypatch.setenv("KMU_PMH_SHORT", "0")
    bases, off = oracle.concat(seqs)
    ctx = lib.Context(0)
    try:
        ctx.profile_reset()
        ctx.profile_enable(True)
        got = np.asarray(ctx.sketch(bases, off, _params()))
        ctx.profile_enable(False)
        prof = ctx.profile_get()
    finally:
        ctx.close()
    return got, {n: v[0] for n, v in prof.items()}


def _both_orders(oracle, monkeypatch, seqs, uq, pmh3a):
    """forward (the leads asked for: the launches are known) and reversed (every read behind the one it stood in front of, other leads)
    against the oracle's rows, computed once: a row depends on its read alone"""
    want = oracle.sketch(*oracle.concat(seqs), _params())
    got, launches = _run(oracle, monkeypatch, seqs)
    assert launches.get("k_multiset_uq", 0) == uq and launches.get("k_sketch_pmh3a", 0) == pmh3a, sorted(launches.items())
    back, _ = _run(oracle, monkeypatch, seqs[::-1])
    for name, rows in (("forward", got), ("reversed", back[::-1])):
        bad = np.nonzero((rows != want).any(axis=1))[0]
        assert bad.size == 0, "%s: rows differ from the oracle: reads %s (lengths %s)" % (name, bad[:8].tolist(), [len(seqs[i]) for i in bad[:8]])
    return want


@pytest.mark.parametrize("lead", LEADS)
def test_no_kmer_and_first_shape_edge(oracle, monkeypatch, lead):
    """a read of k - 1 bases (nk = 0: lst_n = 0, a row of zeros), reads of exactly 10 240 places (the first shape's last) and 10 241 (on
    the redo list, the second shape's through read_list), a short read behind each"""
    b = _Batch(6100 + lead)
    b.at_lead(lead)
    none = b.add(_rnd(b.rng, K - 1))
    b.short()
    last = b.add_span(UQ1_MAX, lead)
    b.short()
    over = b.add_span(UQ1_MAX + 1, lead)
    b.short()
    want = _both_orders(oracle, monkeypatch, b.seqs, uq=2, pmh3a=0)
    assert not want[none].any() and want[last].any() and want[over].any()


@pytest.mark.parametrize("lead", LEADS)
def test_second_shape_edge_and_long_route(oracle, monkeypatch, lead):
    """reads of exactly 20 480 places (the second shape's last) and 20 481 (on its redo list: k_multiset_long's, one launch under the
    timer k_sketch_pmh3a and nothing left for the general kernel), a short read behind each"""
    b = _Batch(6200 + lead)
    b.add_span(UQ2_MAX, lead)
    b.short()
    b.add_span(UQ2_MAX + 1, lead)
    b.short()
    _both_orders(oracle, monkeypatch, b.seqs, uq=2, pmh3a=1)


@pytest.mark.parametrize("lead", LEADS)
def test_too_repetitive_read_is_handed_on(oracle, monkeypatch, lead):
    """3 000 copies of one dinucleotide: 5 970 keys in collision groups, more than either shape collects (1 024, 2 048) and fewer places
    than k_multiset_long takes -- the redo list of all three kernels, then the general kernel; a short read behind it and a read of
    the first shape's in front"""
    b = _Batch(6300 + lead)
    b.add(_rnd(b.rng, 5000))
    b.at_lead(lead)
    rep = b.add(b"AC" * 3000)
    b.short()
    want = _both_orders(oracle, monkeypatch, b.seqs, uq=2, pmh3a=2)
    assert np.unique(want[rep]).size <= 2  # two canonical 31-mers


@pytest.mark.parametrize("lead", LEADS)
def test_empty_read(oracle, monkeypatch, lead):
    """an empty read between two others, in both orders: KMU_E_EMPTY_SEQ"""
    from kmerutils_amd import lib
    b = _Batch(6400 + lead)
    b.add(_rnd(b.rng, 5000))
    b.at_lead(lead)
    b.add(b"")
    b.short()
    for seqs in (b.seqs, b.seqs[::-1]):
        with pytest.raises(lib.KmuError) as e:
            _run(oracle, monkeypatch, seqs)
        assert e.value.code == A.E_EMPTY_SEQ


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("where", ("first read", "first word", "prefetched chunk"))
def test_non_acgt_byte(oracle, monkeypatch, lead, where):
    """an N in the first word of the batch's first read (its workgroup stages it by plain loads), in the first word of a read at the
    lead, and deep in a read whose chunks are requested from the turn of the read in front of it; in both orders: KMU_E_NON_ACGT"""
    from kmerutils_amd import lib
    b = _Batch(6500 + lead)
    if where == "first read":
        s = bytearray(_rnd(b.rng, 4000 + lead))
        s[3] = ord("N")
        b.add(bytes(s))
        b.short()
    else:
        b.add(_rnd(b.rng, 5000))
        b.at_lead(lead)
        s = bytearray(_rnd(b.rng, 6000))
        s[2 if where == "first word" else 2999] = ord("N")
        b.add(bytes(s))
        b.short()
    for seqs in (b.seqs, b.seqs[::-1]):
        with pytest.raises(lib.KmuError) as e:
            _run(oracle, monkeypatch, seqs)
        assert e.value.code == A.E_NON_ACGT

"""k_pmh_points prunes the first points of a read with min(running q_max, tau), tau = m (ln m + c) / W an a-priori guess of the
read's final q_max (W = its k-mer occurrences), verifies the guess per read and does the read again without it where it fails.
The rows must be the oracle's whatever c is: the default, the bound switched off, and a c that makes the guess fail for every
read it is tried on (the path that starts a read over)."""
import math

import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

CASES = (  # (algo, kmer type, k, m, signature)
    (A.ALGO_PROB3A, A.KMER64BIT, 31, 200, A.SIG_U64),
    (A.ALGO_PROB3, A.KMER64BIT, 25, 150, A.SIG_U64),
    (A.ALGO_PROB3A, A.KMER16B32BIT, 16, 64, A.SIG_U32),
    (A.ALGO_PROB3A, A.KMER32BIT, 8, 200, A.SIG_U32),  # the histogram route's lists: every weight large
)


def _reads(oracle):
    rng = np.random.default_rng(4606)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    rnd = lambda n: rng.choice(acgt, size=int(n)).tobytes()  # noqa: E731
    seqs = [rnd(12),          # shorter than k
            rnd(1500),        # under 2 000 k-mers: tau >= 1 at the default c, no bound
            rnd(6000),
            rnd(30000),       # beyond k_multiset_uq's shapes: its list comes from k_sketch_pmh3a
            rnd(45000),       # more than 32 768 list entries: a whole workgroup takes it
            rnd(2000) * 10,   # tandem repeat, 2 000 keys of weight 10
            b"ACGGT" * 3000,  # five keys of weight 3 000: fewer entries than tau wants keys
            rnd(700) * 3 + rnd(3000)]
    return seqs, oracle.concat(seqs)


def _eligible(oracle, seqs, kmer_type, k, m, c):
    """reads the bound is tried on, as (at least, at most): tau < 1 and a list of at least floor(m (ln m + c)) entries.  A list
    holds between the read's distinct keys and its k-mer occurrences (the general multiset kernel lists repeats with weight 0)."""
    tau_num = m * (math.log(m) + c)
    lo = hi = 0
    for s in seqs:
        w = max(0, len(s) - k + 1)
        if w == 0 or not tau_num / w < 1.0:
            continue
        cnt = oracle.Counter(kmer_type, k, 16, 1 << 17)
        b, o = oracle.concat([s])
        cnt.add_reads(b, o)
        lo += cnt.nb_distinct() >= int(tau_num)
        hi += w >= int(tau_num)
    return lo, hi


def _sketch_all(oracle, seqs, bases, off, setting, monkeypatch):
    """every case on a context of its own (the switch is read once per context) -> reads done again, per case"""
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_PMH_SPLIT", "1")  # the two-kernel route also for this small batch
    if setting is None:
        monkeypatch.delenv("KMU_PMH_TAU_C", raising=False)
    else:
        monkeypatch.setenv("KMU_PMH_TAU_C", setting)
    redone = []
    for algo, kmer_type, k, m, sig in CASES:
        ctx = lib.Context(0)
        try:
            p = A.SketchParams(algo, kmer_type, k, m, sig, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)
            ctx.profile_reset()
            ctx.profile_enable(True)
            got = np.asarray(ctx.sketch(bases, off, p))
            ctx.profile_enable(False)
            prof = ctx.profile_get()
        finally:
            ctx.close()
        assert "k_pmh_points" in prof, (setting, k, sorted(prof))
        assert np.array_equal(got, oracle.sketch(bases, off, p)), (setting, algo, kmer_type, k, m)
        redone.append(prof.get("pmh_tau_redone_reads", (0, 0.0))[0])
    return redone


def test_rows_with_the_default_bound(oracle, monkeypatch):
    seqs, (bases, off) = _reads(oracle)
    redone = _sketch_all(oracle, seqs, bases, off, None, monkeypatch)
    for (algo, kmer_type, k, m, sig), n in zip(CASES, redone):
        assert n <= _eligible(oracle, seqs, kmer_type, k, m, 4.6)[1], (k, m, n)


def test_rows_with_the_bound_switched_off(oracle, monkeypatch):
    seqs, (bases, off) = _reads(oracle)
    for setting in ("off", "0"):
        assert _sketch_all(oracle, seqs, bases, off, setting, monkeypatch) == [0] * len(CASES)


def test_rows_when_the_bound_fails_for_every_read(oracle, monkeypatch):
    """c = -4 (m = 200: 1.3 points expected below tau per slot, all 200 slots filled with probability 0.73^200; m = 64, c = -3.5:
    0.66 points per slot): every read the bound is tried on starts over, and its row is still the oracle's."""
    seqs, (bases, off) = _reads(oracle)
    for c in ("-4", "-3.5"):
        redone = _sketch_all(oracle, seqs, bases, off, c, monkeypatch)
        for (algo, kmer_type, k, m, sig), n in zip(CASES, redone):
            lo, hi = _eligible(oracle, seqs, kmer_type, k, m, float(c))
            assert lo >= 3 and lo <= n <= hi, (c, k, m, n, lo, hi)

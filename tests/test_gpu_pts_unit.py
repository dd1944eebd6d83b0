"""k_pmh_points walks the weight-1 prefix of a read's list (the first lst_nu entries, written by k_multiset_uq and k_multiset_long
without a weight word) in a loop of its own: chunks of 64 entries that lie wholly inside the prefix are tested and queued without
weights, their survivors are worked off with h = x, and the general loop takes over at the chunk that straddles lst_nu -- with the
prefix's survivors still in the queue.  While the a-priori bound tau rules pass 1, the running q_max is not refreshed before a share
of the list's chunks (PTS_TAU_HOLD).  The rows must be the oracle's, bit for bit: for every residue of the prefix's length modulo
64, for lists that are all prefix or have none, for the workgroup form and the single wave, with tau on, off, and failing."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

K, M = 31, 200
TAU_MIN_N = 1979  # floor(m (ln m + 4.6)): lists with fewer entries get no bound
ACGT = np.frombuffer(b"ACGT", np.uint8)
SETTINGS = (None, "off", "-4")  # KMU_PMH_TAU_C: the default bound; none; a bound that fails for every read it is tried on (each starts over)


def _params(k=K, m=M, kmer_type=A.KMER64BIT, sig=A.SIG_U64):
    return A.SketchParams(A.ALGO_PROB3A, kmer_type, k, m, sig, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)


def _rnd(rng, n):
    return rng.choice(ACGT, size=int(n)).tobytes()


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
    """int64_hash of the canonical k-mer at every position of the read"""
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
    """base j of the read is made another than base i (where both exist): a planted copy ends where it is meant to end"""
    if 0 <= i and j < len(s) and s[j] == s[i]:
        s[j] = b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]
    return s


def _n_unique(seq, k=K):
    """keys of the read that occur once: the length of its list's weight-1 prefix"""
    _, cnt = np.unique(_keys(seq, k), return_counts=True)
    return int((cnt == 1).sum())


def _run(oracle, monkeypatch, seqs, p, setting=None, pts_long=None):
    """the batch through the two-kernel route on a context of its own (the switches are read once per context) -> (rows, profile)"""
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_PMH_SPLIT", "1")  # the (key, weight) lists also for a small batch
    monkeypatch.delenv("KMU_PMH_PLAIN", raising=False)
    monkeypatch.delenv("KMU_PMH_SHORT", raising=False)
    for name, v in (("KMU_PMH_TAU_C", setting), ("KMU_PMH_PTS_LONG", pts_long)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
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
    assert "k_pmh_points" in prof, sorted(prof)
    return got, prof


def _check(got, want, seqs, what):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: rows differ from the oracle: reads %s (lengths %s)" % (what, bad[:8].tolist(), [len(seqs[i]) for i in bad[:8]])


@pytest.fixture(scope="module")
def sweep(oracle):
    """130 reads of L0, L0 + 1, ... bases, each ending in one 40-base segment three times over (90 k-mers on 40 keys of weight 2 or
    3): the unique count, nk - 90, goes through every residue of 64.  L0 = 700: under the length tau switches on at; 3 000: above."""
    rng = np.random.default_rng(6101)
    seqs = []
    for l0 in (700, 3000):
        for j in range(130):
            s = bytearray(_rnd(rng, l0 + j - 120) + _rnd(rng, 40) * 3)
            seqs.append(bytes(_differ(s, len(s) - 81, len(s) - 121)))  # (the period starts with the segment, not a base earlier)
    nu = np.array([_n_unique(s) for s in seqs])
    assert (nu == np.array([len(s) - K + 1 - 90 for s in seqs])).all()
    for part in (nu[:130], nu[130:]):
        assert set((part % 64).tolist()) == set(range(64))
    assert nu[:130].max() + 40 < TAU_MIN_N < nu[130:].min()
    return seqs, oracle.sketch(*oracle.concat(seqs), _params())


@pytest.mark.parametrize("setting", SETTINGS, ids=("tau_default", "tau_off", "tau_fails"))
def test_every_residue_of_the_prefix_length(oracle, monkeypatch, sweep, setting):
    seqs, want = sweep
    got, prof = _run(oracle, monkeypatch, seqs, _params(), setting)
    _check(got, want, seqs, setting)
    redone = prof.get("pmh_tau_redone_reads", (0, 0.0))[0]
    if setting == "off":
        assert redone == 0
    if setting == "-4":  # tau = 200 (ln 200 - 4) / W < 1 and a list of 259 entries or more: every read of the sweep
        assert redone >= 130, redone


@pytest.fixture(scope="module")
def edge_lists(oracle):
    """lists at the edges of the split: all prefix, no prefix, one key outside it, fewer entries than a chunk, a repeat at the end"""
    rng = np.random.default_rng(6102)
    seqs = [_rnd(rng, 64 * 40 + K - 1),   # all-distinct k-mers, a whole number of chunks: n_u = n, no general chunk
            _rnd(rng, 64 * 40 + 17 + K - 1)]
    assert _n_unique(seqs[0]) == 64 * 40 and _n_unique(seqs[1]) == 64 * 40 + 17
    seqs.append(_rnd(rng, 150) * 6)       # one short tandem repeat: 150 keys of weight 5 or 6, no prefix; pass 2 runs
    seqs.append(_rnd(rng, 2000) * 10)     # ... and one too repetitive for k_multiset_uq: the general kernel's list
    assert _n_unique(seqs[2]) == 0 and _n_unique(seqs[3]) == 0
    s = bytearray(_rnd(rng, 4000))        # exactly one k-mer twice
    s[3000:3000 + K] = s[500:500 + K]
    seqs.append(bytes(_differ(_differ(s, 499, 2999), 500 + K, 3000 + K)))
    assert _n_unique(seqs[4]) == 4000 - K + 1 - 2
    for nk in (1, 63, 64, 65, 127, 128, 129):
        seqs.append(_rnd(rng, nk + K - 1))
    s = bytearray(_rnd(rng, 6000 + K - 1))  # about 6 000 k-mers, the last 200 of them a repeat of earlier ones
    s[-(200 + K - 1):] = s[1000:1000 + 200 + K - 1]
    seqs.append(bytes(_differ(s, 999, len(s) - (200 + K - 1) - 1)))
    assert _n_unique(seqs[-1]) == 6000 - 400
    for nk in range(TAU_MIN_N - 2, TAU_MIN_N + 4):  # lists just under and over tau_min_n entries (tau < 1 from 1 980 k-mers on)
        seqs.append(_rnd(rng, nk + K - 1))
        assert _n_unique(seqs[-1]) == nk
    return seqs, oracle.sketch(*oracle.concat(seqs), _params())


@pytest.mark.parametrize("setting", SETTINGS, ids=("tau_default", "tau_off", "tau_fails"))
def test_edge_lists(oracle, monkeypatch, edge_lists, setting):
    seqs, want = edge_lists
    for order, w in ((seqs, want), (seqs[::-1], want[::-1])):
        got, _ = _run(oracle, monkeypatch, order, _params(), setting)
        _check(got, w, order, setting)


@pytest.mark.parametrize("setting", (None, "-4"), ids=("tau_default", "tau_fails"))
def test_workgroup_form_and_single_waves(oracle, monkeypatch, setting):
    """three reads of about 40 000 distinct k-mers (lists of more than 32 768 entries, nearly all prefix): taken by a workgroup each
    -- wave w on chunks 64 w, 64 w + 256, ..., so the four waves leave the prefix at different chunks -- and by single waves.  (A
    batch that makes the kernel choose single waves by itself needs more than four such reads per workgroup of a grid that the
    batch's own size sets, thousands of them; KMU_PMH_PTS_LONG=0 switches the workgroup form off for the same three reads.)"""
    rng = np.random.default_rng(6103)
    seqs = [_rnd(rng, 40000 + j * 37 + K - 1) for j in range(3)]
    for j in (0, 2):  # a repeat at the end: entries with a weight behind the prefix
        s = bytearray(seqs[j])
        s[-(300 + K - 1):] = s[2000:2000 + 300 + K - 1]
        seqs[j] = bytes(s)
    p = _params()
    want = oracle.sketch(*oracle.concat(seqs), p)
    wg, _ = _run(oracle, monkeypatch, seqs, p, setting)
    single, _ = _run(oracle, monkeypatch, seqs, p, setting, pts_long="0")
    assert np.array_equal(wg, single)
    _check(wg, want, seqs, setting)


def test_sig_u32_every_weight_large(oracle, monkeypatch):
    """k = 8, 32-bit signatures (the histogram route's lists): every weight is large and the prefix is empty"""
    rng = np.random.default_rng(6104)
    seqs = [_rnd(rng, n) for n in (12, 700, 3000, 20000, 45000)] + [b"ACGGT" * 3000]
    p = _params(8, 200, A.KMER32BIT, A.SIG_U32)
    want = oracle.sketch(*oracle.concat(seqs), p)
    for setting in (None, "-4"):
        got, _ = _run(oracle, monkeypatch, seqs, p, setting)
        _check(got, want, seqs, setting)

"""kmu_sketch_groups for OptDens, RevOptDens and HLL: one batched pass (plan, one walk over all groups, finish) in place of a loop
over the groups.  Row g must be, bit for bit, the ALL_SEQS row of the sequences of group g alone -- the oracle's
(sketch_compressedkmer_seqs) and kmu_sketch's --, whatever the cut of the work; the launches of a call depend neither on the
number of groups nor on how many sequences are genome-sized.  Every comparison is exact equality of the raw bytes."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

pytestmark = pytest.mark.gpu

DNA_FH = A.FHASH_CANON_INVHASH
AA_FH = A.FHASH_IDENTITY_RAW
DENS_ALGOS = [(A.ALGO_OPTDENS, A.SIG_F64), (A.ALGO_REVOPTDENS, A.SIG_F32), (A.ALGO_HLL, A.SIG_U16)]
LONG_KMERS = 1 << 20  # kmu_sketch spreads longer sequences over the grid, one launch each


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def raw(x):
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).view(np.uint8)


def offsets_of(lens):
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens, dtype=np.uint64)
    return off


def params(algo, sig, m, kmer_type=A.KMER64BIT, k=21, hasher=A.HASHER_NOHASH, fhash=DNA_FH, flags=0, kind=A.INPUT_ASCII):
    return A.SketchParams(algo, kmer_type, k, m, sig, hasher, fhash, 0, A.MODE_ALL_SEQS, kind, 0, flags)


_LAYOUTS = {}


def mixed_layout(aa=False):
    """a one-read group (50 symbols); 40 reads of 300 .. 3000; an empty group; 300 reads of 60 .. 200; a group of TWO sequences
    above 2^20 k-mers with short ones before, between and behind them; a trailing empty group.  ~2.3 M symbols.
    -> bases, offsets, group_offsets"""
    if aa not in _LAYOUTS:
        rng = np.random.default_rng(0xD5 + aa)
        alpha = synth.AA20 if aa else synth.ACGT
        lens = [50] + [int(L) for L in rng.integers(300, 3000, 40)] + [int(L) for L in rng.integers(60, 201, 300)]
        lens += [700, LONG_KMERS + 12_345, 90, 33, LONG_KMERS + 40, 1500]
        off = offsets_of(lens)
        bases = alpha[rng.integers(0, len(alpha), int(off[-1]))]
        _LAYOUTS[aa] = (bases, off, np.array([0, 1, 41, 41, 341, 347, 347], np.uint64))
    return _LAYOUTS[aa]


def oracle_rows(oracle, bases, off, go, p):
    """row g = the oracle's ALL_SEQS signature of group g alone (offsets re-based to the group's first base)"""
    q = A.SketchParams.from_buffer_copy(p)
    q.mode = A.MODE_ALL_SEQS
    rows = []
    for g in range(len(go) - 1):
        a, b = int(go[g]), int(go[g + 1])
        o = off[a:b + 1]
        sub = bases[int(o[0]):int(o[-1])]
        if sub.size == 0:
            sub = np.zeros(1, np.uint8)
        rows.append(oracle.sketch(np.ascontiguousarray(sub), np.ascontiguousarray(o - o[0]), q)[0])
    return np.stack(rows)


def own_rows(ctx, data, off, go, p, poff=None):
    """row g = kmu_sketch(ALL_SEQS) of group g alone (an empty group: of no sequences)"""
    rows = []
    for g in range(len(go) - 1):
        a, b = int(go[g]), int(go[g + 1])
        if a == b:
            q = A.SketchParams.from_buffer_copy(p)
            q.input_kind = A.INPUT_ASCII  # (no sequences: the row does not depend on how they would have been stored)
            rows.append(np.asarray(ctx.sketch(np.zeros(16, np.uint8), np.zeros(1, np.uint64), q))[0])
        else:
            rows.append(np.asarray(ctx.sketch(data, np.ascontiguousarray(off[a:b + 1]), p,
                                              packed_offsets=None if poff is None else np.ascontiguousarray(poff[a:b + 1])))[0])
    return np.stack(rows)


HLL_DEFAULT, HLL_OTHER = (1.001, 20.0, 65534), (1.05, 5.0, 254)
ORACLE_CASES = [
    # algo, kmer_type, k, m, sig, hasher, fhash, flags, SetSketchParams
    (A.ALGO_OPTDENS, A.KMER64BIT, 21, 1000, A.SIG_F64, A.HASHER_NOHASH, DNA_FH, 0, None),
    (A.ALGO_OPTDENS, A.KMER32BIT, 12, 200, A.SIG_F32, A.HASHER_FNV1A, DNA_FH, 0, None),
    (A.ALGO_REVOPTDENS, A.KMER64BIT, 21, 128, A.SIG_F64, A.HASHER_NOHASH, DNA_FH, 0, None),   # m > the 30 k-mers of group 0
    (A.ALGO_REVOPTDENS, A.KMER64BIT, 21, 2000, A.SIG_F32, A.HASHER_NOHASH, DNA_FH, 0, None),
    (A.ALGO_HLL, A.KMER64BIT, 21, 256, A.SIG_U16, A.HASHER_NOHASH, DNA_FH, 0, HLL_DEFAULT),
    (A.ALGO_HLL, A.KMER64BIT, 21, 4096, A.SIG_U32, A.HASHER_NOHASH, DNA_FH, 0, HLL_OTHER),
    (A.ALGO_HLL, A.KMER64BIT, 25, 1000, A.SIG_U64, A.HASHER_FNV1A, DNA_FH, 0, HLL_DEFAULT),
    (A.ALGO_HLL, A.KMER64BIT, 21, 512, A.SIG_U16, A.HASHER_NOHASH, DNA_FH, 0, HLL_OTHER),
    (A.ALGO_OPTDENS, A.KMERAA64BIT, 7, 512, A.SIG_F64, A.HASHER_NOHASH, AA_FH, 0, None),
    (A.ALGO_HLL, A.KMERAA64BIT, 7, 512, A.SIG_U32, A.HASHER_NOHASH, A.FHASH_VALUE_MASKED, 0, HLL_DEFAULT),
    (A.ALGO_OPTDENS, A.KMER64BIT, 21, 300, A.SIG_F64, A.HASHER_NOHASH, DNA_FH, A.FLAG_RAND08, None),
    (A.ALGO_HLL, A.KMER64BIT, 21, 300, A.SIG_U16, A.HASHER_NOHASH, DNA_FH, A.FLAG_RAND08, HLL_DEFAULT),
    (A.ALGO_OPTDENS, A.KMER64BIT, 21, 9000, A.SIG_F64, A.HASHER_NOHASH, DNA_FH, 0, None),     # 72 KB of bins: the LDS attribute
    (A.ALGO_REVOPTDENS, A.KMER64BIT, 21, 8300, A.SIG_F64, A.HASHER_NOHASH, DNA_FH, 0, None),  # 100 KB with the claims
]


@pytest.mark.parametrize("algo,kmer_type,k,m,sig,hasher,fhash,flags,hll", ORACLE_CASES)
def test_groups_dens_oracle_parity(ctx, oracle, algo, kmer_type, k, m, sig, hasher, fhash, flags, hll):
    aa = kmer_type in (A.KMERAA32BIT, A.KMERAA64BIT)
    bases, off, go = mixed_layout(aa)
    assert int(off[-1]) < 4_000_000 and int((np.diff(off.astype(np.int64)) - k + 1 > LONG_KMERS).sum()) == 2
    p = params(algo, sig, m, kmer_type, k, hasher, fhash, flags)
    try:
        if hll:
            ctx.set_hll_params(*hll)
            oracle.set_hll_params(*hll)
        want = oracle_rows(oracle, bases, off, go, p)
        got = np.asarray(ctx.sketch_groups(bases, off, go, p))
        none = np.asarray(ctx.sketch(np.zeros(16, np.uint8), np.zeros(1, np.uint64), p))
    finally:
        ctx.set_hll_params()
        oracle.set_hll_params()
    assert got.shape == want.shape == (6, m) and got.dtype == want.dtype
    for g in range(6):
        assert np.array_equal(raw(got[g]), raw(want[g])), "group %d" % g
    # the empty groups: the device's own ALL_SEQS row of no sequences -- undensified "large" bins, zero registers
    assert np.array_equal(raw(got[2]), raw(none[0])) and np.array_equal(raw(got[5]), raw(none[0]))


@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
@pytest.mark.parametrize("where", ["host", "device"])
def test_groups_dens_packed_and_device(ctx, algo, sig, where):
    """PACKED2 input, host and device memory, the genome-sized sequences included: the rows of kmu_sketch(ALL_SEQS) per group"""
    import torch
    bases, off, go = mixed_layout()
    p = params(algo, sig, 333, kind=A.INPUT_PACKED2)
    data, poff = ctx.pack2b(bases, off)
    data = np.ascontiguousarray(np.concatenate([data, np.zeros(16, np.uint8)]))
    want = own_rows(ctx, data, off, go, p, poff)
    if where == "device":
        dev = torch.device("cuda", 0)
        got = ctx.sketch_groups(torch.from_numpy(data).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                                torch.from_numpy(go.astype(np.int64)).to(dev), p, packed_offsets=torch.from_numpy(poff.astype(np.int64)).to(dev))
        assert got.is_cuda
    else:
        got = ctx.sketch_groups(data, off, go, p, packed_offsets=poff)
    assert np.array_equal(raw(got).reshape(6, -1), raw(want).reshape(6, -1))
    # ... and ASCII on the same side gives the same rows
    if where == "device":
        got_a = ctx.sketch_groups(torch.from_numpy(bases).to(dev), torch.from_numpy(off.astype(np.int64)).to(dev),
                                  torch.from_numpy(go.astype(np.int64)).to(dev), params(algo, sig, 333))
    else:
        got_a = ctx.sketch_groups(bases, off, go, params(algo, sig, 333))
    assert np.array_equal(raw(got_a), raw(got))


def launches(ctx, fn):
    ctx.profile_reset()
    fn()
    prof = ctx.profile_get()
    n = sum(c for c, _ in prof.values())
    assert n > 0
    return n, prof


@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
def test_dens_launches_do_not_grow_with_groups(ctx, algo, sig):
    """one batched pass, not a loop: as many launches (of all kernels, the fill and the finish among them) for 512 groups as
    for 8 groups of the same 4 M bases"""
    bases, off = synth.uniform_reads(8192, 512, 0x8E)
    n = len(off) - 1
    p = params(algo, sig, 64)
    counts = []
    ctx.profile_enable(True)
    try:
        for n_groups in (8, 512):
            go = np.arange(0, n + 1, n // n_groups, dtype=np.uint64)
            counts.append(launches(ctx, lambda: ctx.sketch_groups(bases, off, go, p)))
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    assert counts[0][0] == counts[1][0], counts


@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
def test_dens_launches_do_not_grow_with_long_sequences(ctx, algo, sig):
    """the same 4.2 M bases as three sequences of 1.4 M (each above 2^20 k-mers) and as 4 096 sequences of 1 025, one group each:
    the same launches, and each way the row of kmu_sketch(ALL_SEQS)"""
    rng = np.random.default_rng(0x10A6)
    total = 4096 * 1025
    bases = synth.ACGT[rng.integers(0, 4, total)]
    off_long = np.array([0, 1_400_000, 2_800_000, total], np.uint64)
    off_short = np.arange(0, total + 1, 1025, dtype=np.uint64)
    p = params(algo, sig, 64)
    counts = []
    ctx.profile_enable(True)
    try:
        for off in (off_long, off_short):
            go = np.array([0, len(off) - 1], np.uint64)
            got = []
            counts.append(launches(ctx, lambda: got.append(np.asarray(ctx.sketch_groups(bases, off, go, p)))))
            assert np.array_equal(raw(got[0]), raw(np.asarray(ctx.sketch(bases, off, p))))
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    assert counts[0][0] == counts[1][0], counts


@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
def test_dens_groups_are_independent(ctx, algo, sig):
    bases, off, go = mixed_layout()
    n = len(off) - 1
    p = params(algo, sig, 128)
    a = np.asarray(ctx.sketch_groups(bases, off, go, p))
    b = np.asarray(ctx.sketch_groups(bases, off, go, p))
    assert np.array_equal(raw(a), raw(b))  # two identical calls: identical bytes
    assert np.array_equal(raw(a), raw(own_rows(ctx, bases, off, go, p)))
    # the OTHER sequences grouped differently: groups 0 and 1 keep their rows, the long group's sequences regrouped do not disturb them
    go2 = np.array([0, 1, 41, 100, 101, 250, 341, 343, n], np.uint64)
    c = np.asarray(ctx.sketch_groups(bases, off, go2, p))
    assert np.array_equal(raw(a[0]), raw(c[0])) and np.array_equal(raw(a[1]), raw(c[1]))
    assert np.array_equal(raw(c), raw(own_rows(ctx, bases, off, go2, p)))
    # the sequences of a group in another order (the long ones too): the same minima / maxima, the same row
    L = np.diff(off.astype(np.int64))
    order = np.arange(n)
    rng = np.random.default_rng(3)
    order[1:41] = 1 + rng.permutation(40)
    order[41:341] = 41 + rng.permutation(300)
    order[341:347] = 341 + rng.permutation(6)
    pb = np.concatenate([bases[int(off[i]):int(off[i + 1])] for i in order])
    shuffled = np.asarray(ctx.sketch_groups(pb, offsets_of(L[order]), go, p))
    assert np.array_equal(raw(a), raw(shuffled))


@pytest.mark.parametrize("m", [64, 1024])
def test_hll_tiny_group_behind_a_large_one(ctx, oracle, m):
    """a group of very high cardinality immediately before a tiny one: the tiny group's registers are its own ALL_SEQS row.
    (A K_low carried across the group change would prune the tiny group's updates.)"""
    rng = np.random.default_rng(0x4C0 + m)
    lens = [900_000, 600_000, 30, 25, 400_000, 21]
    off = offsets_of(lens)
    bases = synth.ACGT[rng.integers(0, 4, int(off[-1]))]
    go = np.array([0, 2, 3, 4, 5, 6], np.uint64)
    p = params(A.ALGO_HLL, A.SIG_U16, m)
    got = np.asarray(ctx.sketch_groups(bases, off, go, p))
    want = oracle_rows(oracle, bases, off, go, p)
    for g in range(5):
        assert np.array_equal(raw(got[g]), raw(want[g])), "group %d" % g
    assert got[1].max() > 0 and np.array_equal(raw(got), raw(own_rows(ctx, bases, off, go, p)))


def _code(fn):
    from kmerutils_amd.lib import KmuError
    with pytest.raises(KmuError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
def test_dens_group_errors(ctx, algo, sig):
    """what kmu_sketch reports, kmu_sketch_groups reports, on host and on device; a correct call after each gives correct rows"""
    import torch
    dev = torch.device("cuda", 0)
    k = 21
    rng = np.random.default_rng(0xE77)
    lens = [300, 15, 2000, 40, 5000, 700, 12, 900]
    off = offsets_of(lens)
    bases = synth.ACGT[rng.integers(0, 4, int(off[-1]))]
    go = np.array([0, 3, 3, 6, 8], np.uint64)
    p = params(algo, sig, 96)
    want = own_rows(ctx, bases, off, go, p)

    def to_dev(x):
        return torch.from_numpy(x if x.dtype == np.uint8 else x.astype(np.int64)).to(dev)

    def both(b, o, g, q, expect):
        if expect != A.E_BAD_ARG:  # (group_offsets are not kmu_sketch's)
            assert _code(lambda: ctx.sketch(b, o, q)) == expect
        assert _code(lambda: ctx.sketch_groups(b, o, g, q)) == expect
        assert np.array_equal(raw(ctx.sketch_groups(bases, off, go, p)), raw(want))
        assert _code(lambda: ctx.sketch_groups(to_dev(b), to_dev(o), to_dev(g), q)) == expect
        assert np.array_equal(raw(ctx.sketch_groups(to_dev(bases), to_dev(off), to_dev(go), p)), raw(want))
    # N in a sequence shorter than k (it starts no k-mer: only the validation sees it)
    nb = bases.copy()
    nb[int(off[1]) + 7] = ord("N")
    both(nb, off, go, p, A.E_NON_ACGT)
    nb = bases.copy()
    nb[int(off[6]) + 11] = ord("N")
    both(nb, off, go, p, A.E_NON_ACGT)
    # N in the last k - 1 bases of a sequence: in no k-mer's first base
    for s in (2, 4):
        for back in (1, k - 1):
            nb = bases.copy()
            nb[int(off[s + 1]) - back] = ord("N")
            both(nb, off, go, p, A.E_NON_ACGT)
    # an empty sequence in the middle of a group
    eoff = off.copy()
    eoff[5] = eoff[4]  # sequence 4 is empty
    both(bases, eoff, go, p, A.E_EMPTY_SEQ)
    # malformed group_offsets (host: checked on the host; device: checked by the plan kernel before anything reads through them)
    for bad in ([1, 3, 3, 6, 8], [0, 4, 3, 6, 8], [0, 3, 3, 6, 7], [0, 3, 3, 6, 9], [0, 3, 3, 6, 1 << 40], [0, 3, 1 << 50, 6, 8]):
        both(bases, off, np.array(bad, np.uint64), p, A.E_BAD_ARG)
    # a sketch that does not fit the LDS
    both(bases, off, go, params(algo, sig, 21000), A.E_UNSUPPORTED)
    # amino acids: a residue outside the alphabet, in a sequence shorter than k
    alens = [200, 5, 300]
    aoff = offsets_of(alens)
    ab = synth.AA20[rng.integers(0, 20, int(aoff[-1]))]
    ab[int(aoff[1]) + 2] = ord("B")
    pa = params(algo, sig, 96, A.KMERAA64BIT, 7, fhash=AA_FH)
    ago = np.array([0, 2, 3], np.uint64)
    assert _code(lambda: ctx.sketch(ab, aoff, pa)) == _code(lambda: ctx.sketch_groups(ab, aoff, ago, pa)) == A.E_BAD_ALPHABET
    assert np.array_equal(raw(ctx.sketch_groups(bases, off, go, p)), raw(want))

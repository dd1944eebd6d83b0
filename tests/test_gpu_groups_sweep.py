"""Seeded sweep over the parameter space of kmu_sketch_groups (small inputs), the counterpart of tests/test_gpu_fuzz.py for the
grouped entry point.  tests/test_gpu_groups.py and tests/test_gpu_groups_dens.py pin hand-picked k, m, hashers and flags on two
layouts; here every seed draws the algorithm (ProbMinHash3a / 3, SuperMinHash / 2, OptDens, RevOptDens, HLL), the k-mer type and
every k it allows, sketch sizes from 2 to 4000, signature type, hasher, fhash, FLAG_RAND08, the HLL parameters, 1 .. 60 sequences
of four kinds (reads shorter than k, reads of 20 .. 60 k, repeats), 1 .. 25 ragged groups with empty ones among them, every fourth
seed a group made only of reads shorter than k, ASCII or PACKED2 input, host or device memory.  Every row is compared byte for
byte with the oracle's ALL_SEQS signature of its group alone; a second call with the sequences permuted inside every group must
give the same rows.  test_sweep_composition needs no GPU: it walks the same seeds with the oracle alone and checks that the sweep
reaches what this paragraph says."""
import os

import numpy as np
import pytest

from kmerutils_amd import _abi as A

# KMU_FUZZ_SCALE=10 runs ten times as many seeds (an occasional long run; the default keeps the suite short)
SCALE = int(os.environ.get("KMU_FUZZ_SCALE", "1"))
N_SEEDS = 48
BASE_SEED = 6000

ACGT_MIXED = np.frombuffer(b"ACGTacgt", np.uint8)
ACGT = np.frombuffer(b"ACGT", np.uint8)
AA20 = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
HLL_DEFAULT, HLL_OTHER = (1.001, 20.0, 65534), (1.05, 5.0, 254)
ALGOS = [A.ALGO_PROB3A, A.ALGO_PROB3A, A.ALGO_PROB3, A.ALGO_SUPER, A.ALGO_SUPER2, A.ALGO_OPTDENS, A.ALGO_REVOPTDENS, A.ALGO_HLL]


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _reads(rng, n, kind, aa):
    """the four kinds of test_gpu_fuzz.py's _reads, over either alphabet"""
    unit_alpha, alpha = (AA20, AA20) if aa else (ACGT, ACGT_MIXED)
    out = []
    for i in range(n):
        if kind == "short":
            L = int(rng.integers(1, 60))
        elif kind == "long":
            L = int(rng.integers(1, 40)) if i % 3 else int(rng.integers(20_000, 60_000))
        else:
            L = int(rng.integers(50, 4000))
        if kind == "repeat" and i % 2 == 0:
            unit = rng.choice(unit_alpha, size=int(rng.integers(1, 9))).tobytes()
            out.append((unit * (L // len(unit) + 1))[:L])
        else:
            out.append(rng.choice(alpha, size=L).tobytes())
    return out


def _kmer_choice(rng):
    t = int(rng.choice([A.KMER32BIT, A.KMER16B32BIT, A.KMER64BIT]))
    if t == A.KMER32BIT:
        return t, int(rng.integers(1, 15))
    if t == A.KMER16B32BIT:
        return t, 16
    return t, int(rng.integers(15, 32))


def draw(seed):
    """the configuration of a seed: params (host ASCII), HLL parameters or None, the groups (lists of sequences), whether one of
    them was appended as the all-short group, the input kind and side, the seed of the permutation"""
    rng = np.random.default_rng(BASE_SEED + seed)
    algo = int(rng.choice(ALGOS))
    aa = bool(rng.random() < 0.2)
    if aa:
        kmer_type = int(rng.choice([A.KMERAA32BIT, A.KMERAA64BIT]))
        k = int(rng.integers(1, 7 if kmer_type == A.KMERAA32BIT else 13))
        fhash = int(rng.choice([A.FHASH_IDENTITY_RAW, A.FHASH_VALUE_MASKED, A.FHASH_INVHASH_RAW]))
    else:
        kmer_type, k = _kmer_choice(rng)
        fhash = int(rng.choice([A.FHASH_IDENTITY_RAW, A.FHASH_VALUE_MASKED, A.FHASH_CANON_RAW, A.FHASH_CANON_INVHASH,
                                A.FHASH_INVHASH_RAW, A.FHASH_CANON_VALUE, A.FHASH_CANON_NTHASH]))
        if fhash == A.FHASH_CANON_NTHASH and kmer_type != A.KMER64BIT:
            fhash = A.FHASH_CANON_INVHASH  # ntHash is a 64-bit value
    w32 = A.kmer_val_bytes(kmer_type) == 4
    m = int(rng.choice([2, 7, 64, 100, 200, 333, 1000, 4000]))
    if algo == A.ALGO_SUPER:
        m = min(m, 1000)
    if algo in (A.ALGO_PROB3A, A.ALGO_PROB3):
        sig, hasher = (A.SIG_U32 if w32 else A.SIG_U64), A.HASHER_NOHASH
    else:
        sig = int(rng.choice({A.ALGO_SUPER2: [A.SIG_U32, A.SIG_U64], A.ALGO_HLL: [A.SIG_U16, A.SIG_U32, A.SIG_U64]}
                             .get(algo, [A.SIG_F32, A.SIG_F64])))
        hasher = int(rng.choice([A.HASHER_NOHASH, A.HASHER_FNV1A]))
    flags = A.FLAG_RAND08 if rng.random() < 0.25 else 0
    hll = None
    if algo == A.ALGO_HLL:
        hll = HLL_OTHER if rng.random() < 0.5 else HLL_DEFAULT
    seqs = _reads(rng, int(rng.integers(1, 61)), str(rng.choice(["normal", "short", "long", "repeat"])), aa)
    n_groups = int(rng.integers(1, 26))
    sizes = rng.multinomial(len(seqs), np.full(n_groups, 1.0 / n_groups))
    cuts = np.concatenate([[0], np.cumsum(sizes)])
    groups = [seqs[int(cuts[g]):int(cuts[g + 1])] for g in range(n_groups)]
    all_short = seed % 4 == 3 and k > 1  # (no read is shorter than k = 1)
    if all_short:
        alpha = AA20 if aa else ACGT
        groups.append([rng.choice(alpha, size=int(rng.integers(1, k))).tobytes() for _ in range(int(rng.integers(1, 5)))])
    packed = bool(rng.random() < 0.5) and not aa
    device = bool(rng.random() < 0.5)
    p = A.SketchParams(algo, kmer_type, k, m, sig, hasher, fhash, 0, A.MODE_ALL_SEQS, A.INPUT_ASCII, A.MEM_HOST, flags)
    return dict(p=p, hll=hll, groups=groups, all_short=all_short, packed=packed, device=device, perm_seed=int(rng.integers(1 << 30)))


def expected(oracle, cfg):
    """row g = the oracle's ALL_SEQS signature of group g alone; OracleError where the oracle refuses the configuration"""
    rows = []
    try:
        if cfg["hll"]:
            oracle.set_hll_params(*cfg["hll"])
        for grp in cfg["groups"]:
            bases, off = oracle.concat(grp)
            rows.append(oracle.sketch(bases, off, cfg["p"])[0])
    finally:
        oracle.set_hll_params()
    return np.stack(rows)


def call(ctx, oracle, cfg, groups):
    """one kmu_sketch_groups call on `groups`, with the input kind and on the side the seed drew"""
    bases, off = oracle.concat([s for grp in groups for s in grp])
    go = np.zeros(len(groups) + 1, np.uint64)
    go[1:] = np.cumsum([len(grp) for grp in groups])
    p = A.SketchParams.from_buffer_copy(cfg["p"])
    data, poff = bases, None
    if cfg["packed"]:
        p.input_kind = A.INPUT_PACKED2
        data, poff = ctx.pack2b(bases, off)
        data = np.ascontiguousarray(np.concatenate([data, np.zeros(16, np.uint8)]))
    if cfg["device"]:
        import torch
        dev = torch.device("cuda", 0)
        data, off, go = (torch.from_numpy(x if x.dtype == np.uint8 else x.astype(np.int64)).to(dev) for x in (data, off, go))
        if poff is not None:
            poff = torch.from_numpy(poff.astype(np.int64)).to(dev)
    got = ctx.sketch_groups(data, off, go, p, packed_offsets=poff)
    return np.asarray(got.cpu()) if cfg["device"] else np.asarray(got)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(N_SEEDS * SCALE))
def test_groups_sweep(ctx, oracle, seed):
    from kmerutils_amd.lib import KmuError
    cfg = draw(seed)
    p = cfg["p"]
    what = (p.algo, p.kmer_type, p.kmer_size, p.sketch_size, p.sig_type, p.hasher, p.fhash, p.flags, cfg["hll"], cfg["packed"], cfg["device"])
    try:
        if cfg["hll"]:
            ctx.set_hll_params(*cfg["hll"])
        try:
            want = expected(oracle, cfg)
        except oracle.OracleError as e:  # the device must refuse with the same status
            with pytest.raises(KmuError) as g:
                call(ctx, oracle, cfg, cfg["groups"])
            assert A.STATUS_NAMES[g.value.code] == str(e), what
            return
        got = call(ctx, oracle, cfg, cfg["groups"])
        assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, what
        for g in range(len(want)):
            assert got[g].tobytes() == want[g].tobytes(), ("group %d of %d" % (g, len(want)), what)
        # the sequences of every group in another order: the same multisets, minima and maxima, the same rows
        rng = np.random.default_rng(cfg["perm_seed"])
        shuffled = [[grp[i] for i in rng.permutation(len(grp))] for grp in cfg["groups"]]
        again = call(ctx, oracle, cfg, shuffled)
        assert again.tobytes() == got.tobytes(), ("permuted", what)
    finally:
        ctx.set_hll_params()


def test_sweep_composition(oracle):
    """no GPU: the 48 seeds of the default run with the oracle alone.  At most one in ten ends in a refusal, and the accepted ones
    hold every algorithm, both input kinds, both sides, an empty group and a group made only of reads shorter than k."""
    refused, algos, kinds, sides, empty, short, aa = 0, set(), set(), set(), 0, 0, 0
    for seed in range(N_SEEDS):
        cfg = draw(seed)
        again = draw(seed)  # (a function of the seed alone)
        assert again["groups"] == cfg["groups"] and bytes(again["p"]) == bytes(cfg["p"]) and again["perm_seed"] == cfg["perm_seed"]
        try:
            rows = expected(oracle, cfg)
        except oracle.OracleError:
            refused += 1
            continue
        p = cfg["p"]
        assert rows.shape == (len(cfg["groups"]), p.sketch_size)
        algos.add(p.algo)
        kinds.add(cfg["packed"])
        sides.add(cfg["device"])
        empty += any(len(grp) == 0 for grp in cfg["groups"])
        aa += p.kmer_type in (A.KMERAA32BIT, A.KMERAA64BIT)
        if cfg["all_short"]:
            assert all(len(s) < p.kmer_size for s in cfg["groups"][-1]) and len(cfg["groups"][-1]) >= 1
            short += 1
    assert refused * 10 <= N_SEEDS, refused
    assert algos == set(ALGOS)
    assert kinds == {False, True} and sides == {False, True}
    assert empty >= 1 and short >= 1 and aa >= 1

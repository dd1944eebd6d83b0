"""kmu_sketch_groups at the sizes where its kernels change path.  tests/test_gpu_groups.py and tests/test_gpu_groups_dens.py use at
most 512 groups and groups of at most ~2 M k-mers: every kernel of kmu_sketch_groups.hip runs there on the first trip of its loops
only.  This file adds two fixed layouts that reach what they leave out:

  layout A, "many groups" (4 100 groups, ~1.5 M symbols, DNA and an amino-acid twin): the second trip of k_group_plan's group loop
      (the carry of grp_block_scan across trips, n_groups >= 1025), workgroups of k_grp_bounds and k_grp_dens_finish that take a
      second, third ... group (grids of at most 2 x CUs and 8 x CUs workgroups), single-leaf and multi-leaf groups on both sides of
      every one of these bounds, empty groups next to group 0, at the end and every 97 groups, a group made only of reads shorter
      than k; and, for OptDens / RevOptDens / HLL, n_groups == n_seq (a group change at every sequence, dozens inside one tile of
      4 096 bases, reads shorter than k among them).
  layout B, "large groups" (~22.6 Mbases, DNA): a group of 16.9 M 21-mers (pmh_leaf_bits 13 > GRP_LDS_BITS: the key-by-key branch of
      k_grp_hist and k_grp_scatter; equal keys 3 Mbases apart must still meet in one leaf), a group of 4.3 M (2^11 leaves: the
      second trip of k_grp_bounds' scan), a group of one 1.1 Mbase sequence (more than 64 SuperMinHash chunks: the second trip of
      k_grp_chunk_offsets), and a dens tile above GD_TILE_MIN.

Rows are compared, as raw bytes, with the oracle's ALL_SEQS signature of every group alone and (layout B) with kmu_sketch(ALL_SEQS)
of every group alone, which partitions with other kernels (kmu_sketch.hip) -- a second, independent witness.  All four cases of
layout B keep their oracle pass (one to four seconds of CPU each), cached by case for the tests that share it.
test_layouts_reach_the_thresholds needs no GPU: it fails on any machine if a layout is trimmed below a threshold."""
import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

gpu = pytest.mark.gpu

DNA_FH = A.FHASH_CANON_INVHASH
AA_FH = A.FHASH_IDENTITY_RAW


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


def assemble(groups):
    """list of groups, each a list of sequences -> bases, offsets, group_offsets"""
    seqs = [s for grp in groups for s in grp]
    return np.concatenate(seqs), offsets_of([s.size for s in seqs]), offsets_of([len(grp) for grp in groups])


def group_kmers(off, go, k):
    """k-mers of every group"""
    nk = np.maximum(np.diff(off.astype(np.int64)) - k + 1, 0)
    c = np.concatenate([[0], np.cumsum(nk)])
    return c[go[1:].astype(np.int64)] - c[go[:-1].astype(np.int64)]


def params(algo, kmer_type, k, m, sig, hasher=A.HASHER_NOHASH, fhash=DNA_FH, kind=A.INPUT_ASCII, mode=A.MODE_ALL_SEQS):
    return A.SketchParams(algo, kmer_type, k, m, sig, hasher, fhash, 0, mode, kind, 0, 0)


def oracle_rows(oracle, bases, off, go, p):
    """row g = the oracle's ALL_SEQS signature of group g alone (offsets re-based to the group's first base)"""
    q = A.SketchParams.from_buffer_copy(p)
    q.mode = A.MODE_ALL_SEQS
    q.input_kind = A.INPUT_ASCII
    rows = []
    for g in range(len(go) - 1):
        a, b = int(go[g]), int(go[g + 1])
        o = off[a:b + 1]
        sub = bases[int(o[0]):int(o[-1])]
        if sub.size == 0:
            sub = np.zeros(1, np.uint8)
        rows.append(oracle.sketch(np.ascontiguousarray(sub), np.ascontiguousarray(o - o[0]), q)[0])
    return np.stack(rows)


def own_rows(ctx, bases, off, go, p):
    """row g = kmu_sketch(ALL_SEQS) of group g alone (an empty group: of no sequences)"""
    rows = []
    for g in range(len(go) - 1):
        a, b = int(go[g]), int(go[g + 1])
        if a == b:
            rows.append(np.asarray(ctx.sketch(np.zeros(16, np.uint8), np.zeros(1, np.uint64), p))[0])
        else:
            rows.append(np.asarray(ctx.sketch(bases, np.ascontiguousarray(off[a:b + 1]), p))[0])
    return np.stack(rows)


def assert_rows(got, want, what=""):
    got, want = np.asarray(got.cpu() if hasattr(got, "cpu") else got), np.asarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (got.shape, want.shape, got.dtype, want.dtype)
    n = got.shape[0]
    bad = np.flatnonzero((raw(got).reshape(n, -1) != raw(want).reshape(n, -1)).any(axis=1))
    assert bad.size == 0, "%s: %d rows differ, the first are groups %s" % (what, bad.size, bad[:8].tolist())


def to_dev(x):
    import torch
    return torch.from_numpy(x if x.dtype == np.uint8 else x.astype(np.int64)).to(torch.device("cuda", 0))


# ---- layout A: many groups -----------------------------------------------------------------------------------------------------
A_GROUPS = 4100
# groups of 6 000 .. 20 000 k-mers (2 .. 8 leaves) on both sides of 512 (k_grp_bounds' grid on 256 CUs), 1 024 (k_group_plan's
# trip) and 2 048 (k_grp_dens_finish's largest grid on 256 CUs)
A_MULTI = (7, 300, 511, 512, 800, 1023, 1025, 1500, 2047, 2049, 3000, 4098)
A_SHORT = 2500  # the group made only of reads shorter than k (3 .. 6 symbols; every k of this file is >= 7)
A_EMPTY = frozenset([1, A_GROUPS - 1] + [g for g in range(A_GROUPS) if g % 97 == 96])
_LAYOUT_A = {}


def layout_a(aa=False):
    """-> bases, offsets, group_offsets (fixed seed; the amino-acid twin comes from the same recipe)"""
    if aa not in _LAYOUT_A:
        rng = np.random.default_rng(0xA6 + aa)
        alpha = synth.AA20 if aa else synth.ACGT
        small = alpha[rng.integers(0, len(alpha), 4000)]    # the multi-leaf groups are cut from it: their keys repeat
        pool = alpha[rng.integers(0, len(alpha), 60_000)]

        def cut(src, L):
            s = int(rng.integers(0, src.size - L))
            return src[s:s + L]
        groups = []
        for g in range(A_GROUPS):
            if g in A_EMPTY:
                groups.append([])
            elif g in A_MULTI:
                grp, left = [], int(rng.integers(7000, 16000))
                while left > 0:
                    grp.append(cut(small, int(rng.integers(1000, 3001))))
                    left -= grp[-1].size
                groups.append(grp)
            elif g == A_SHORT:
                groups.append([cut(pool, int(L)) for L in rng.integers(3, 7, 5)])
            else:
                groups.append([cut(pool, int(L)) for L in rng.integers(40, 301, int(rng.integers(1, 4)))])
        _LAYOUT_A[aa] = assemble(groups)
    return _LAYOUT_A[aa]


A_CASES = {
    # name: aa, params
    "prob3a_u64_k21": (False, params(A.ALGO_PROB3A, A.KMER64BIT, 21, 100, A.SIG_U64)),
    "prob3a_u32_k12": (False, params(A.ALGO_PROB3A, A.KMER32BIT, 12, 64, A.SIG_U32)),
    "prob3_u64_k21": (False, params(A.ALGO_PROB3, A.KMER64BIT, 21, 64, A.SIG_U64)),
    "super_f32_fnv": (False, params(A.ALGO_SUPER, A.KMER64BIT, 21, 100, A.SIG_F32, A.HASHER_FNV1A)),
    "super2_u64": (False, params(A.ALGO_SUPER2, A.KMER64BIT, 21, 128, A.SIG_U64)),
    "optdens_f64": (False, params(A.ALGO_OPTDENS, A.KMER64BIT, 21, 200, A.SIG_F64)),
    "revoptdens_f32": (False, params(A.ALGO_REVOPTDENS, A.KMER64BIT, 21, 128, A.SIG_F32)),
    "hll_u16": (False, params(A.ALGO_HLL, A.KMER64BIT, 21, 256, A.SIG_U16)),
    "aa_super_f64_k12": (True, params(A.ALGO_SUPER, A.KMERAA64BIT, 12, 128, A.SIG_F64, fhash=AA_FH)),
    "aa_optdens_k7": (True, params(A.ALGO_OPTDENS, A.KMERAA64BIT, 7, 128, A.SIG_F64, fhash=AA_FH)),
}
A_DNA_CASES = [name for name, (aa, _) in A_CASES.items() if not aa]
_HOST_A = {}


def host_rows_a(ctx, name):
    """the host ASCII call of a case on layout A, made once"""
    if name not in _HOST_A:
        aa, p = A_CASES[name]
        bases, off, go = layout_a(aa)
        _HOST_A[name] = np.asarray(ctx.sketch_groups(bases, off, go, p))
    return _HOST_A[name]


@gpu
@pytest.mark.parametrize("name", list(A_CASES))
def test_many_groups_oracle_parity(ctx, oracle, name):
    aa, p = A_CASES[name]
    bases, off, go = layout_a(aa)
    got = host_rows_a(ctx, name)
    want = oracle_rows(oracle, bases, off, go, p)
    assert got.shape == (A_GROUPS, p.sketch_size)
    assert_rows(got, want, name)
    # the empty groups: the device's own ALL_SEQS row of no sequences
    none = np.asarray(ctx.sketch(np.zeros(16, np.uint8), np.zeros(1, np.uint64), p))
    empty = sorted(A_EMPTY)
    assert_rows(got[empty], np.repeat(none, len(empty), axis=0), name + ", empty groups")


@gpu
@pytest.mark.parametrize("name", A_DNA_CASES)
def test_many_groups_device_and_packed(ctx, name):
    """device-resident input and PACKED2 input, on either side: the bytes of the host ASCII call"""
    _, p = A_CASES[name]
    bases, off, go = layout_a()
    want = host_rows_a(ctx, name)
    got = ctx.sketch_groups(to_dev(bases), to_dev(off), to_dev(go), p)
    assert got.is_cuda
    assert_rows(got, want, name + ", device ASCII")
    data, poff = ctx.pack2b(bases, off)
    data = np.ascontiguousarray(np.concatenate([data, np.zeros(16, np.uint8)]))
    q = A.SketchParams.from_buffer_copy(p)
    q.input_kind = A.INPUT_PACKED2
    assert_rows(ctx.sketch_groups(data, off, go, q, packed_offsets=poff), want, name + ", host PACKED2")
    got = ctx.sketch_groups(to_dev(data), to_dev(off), to_dev(go), q, packed_offsets=to_dev(poff))
    assert got.is_cuda
    assert_rows(got, want, name + ", device PACKED2")


DENS_ALGOS = [(A.ALGO_OPTDENS, A.SIG_F64), (A.ALGO_REVOPTDENS, A.SIG_F32), (A.ALGO_HLL, A.SIG_U16)]
_SHORT_READS = []


def short_reads():
    """3 000 reads of 30 .. 120 bases: ~55 sequences, and as many groups, in a tile of 4 096 bases; some shorter than k = 21"""
    if not _SHORT_READS:
        rng = np.random.default_rng(0x5407)
        lens = rng.integers(30, 121, 3000)
        lens[::17] = rng.integers(1, 21, lens[::17].size)
        off = offsets_of(lens)
        _SHORT_READS.append((synth.ACGT[rng.integers(0, 4, int(off[-1]))], off))
    return _SHORT_READS[0]


@gpu
@pytest.mark.parametrize("algo,sig", DENS_ALGOS)
def test_dens_one_sequence_per_group(ctx, oracle, algo, sig):
    """n_groups == n_seq for OptDens / RevOptDens / HLL: the rows of MODE_PER_SEQ, and the oracle's per read"""
    bases, off = synth.ont_reads(300, 300_000, 0x715)
    n = len(off) - 1
    p = params(algo, A.KMER64BIT, 21, 100, sig, mode=A.MODE_PER_SEQ)
    got = ctx.sketch_groups(bases, off, np.arange(n + 1, dtype=np.uint64), p)
    assert_rows(got, ctx.sketch(bases, off, p), "ont reads")
    bases, off = short_reads()
    n = len(off) - 1
    assert n == 3000 and int((np.diff(off.astype(np.int64)) < 21).sum()) >= 100
    got = ctx.sketch_groups(bases, off, np.arange(n + 1, dtype=np.uint64), p)
    assert_rows(got, oracle.sketch(bases, off, p), "short reads")


# ---- layout B: large groups ----------------------------------------------------------------------------------------------------
B_K = 21
B_TINY, B_HUGE, B_EMPTY, B_4M, B_ONE, B_TAIL = range(6)
_LAYOUT_B = {}


def _b_groups():
    if "groups" not in _LAYOUT_B:
        rng = np.random.default_rng(0xB16)

        def rnd(n):
            return synth.ACGT[rng.integers(0, 4, int(n), dtype=np.uint8)]

        def reads(n, lo, hi):
            return [rnd(L) for L in rng.integers(lo, hi + 1, n)]
        # a 3 Mbase genome tiled four times with 1 % substitutions: equal keys occur 3, 6 and 9 Mbases apart
        tiled = np.tile(rnd(3_000_000), 4)
        mut = np.flatnonzero(rng.random(tiled.size) < 0.01)
        tiled[mut] = synth.ACGT[rng.integers(0, 4, mut.size)]
        huge = reads(50, 100, 3000) + [tiled] + reads(50, 100, 3000) + [rnd(1_900_000)] + reads(30, 100, 3000) + [rnd(1_600_000)]
        huge += reads(20, 100, 3000) + [rnd(1_300_000)] + reads(50, 100, 3000)
        four = reads(10, 60, 400) + [rnd(2_500_000)] + reads(10, 60, 400) + [rnd(1_800_000)] + reads(10, 60, 400)
        _LAYOUT_B["groups"] = [[rnd(50)], huge, [], four, [rnd(1_100_000)], reads(30, 25, 200)]
    return _LAYOUT_B["groups"]


B_ORDER = (B_TINY, B_HUGE, B_EMPTY, B_4M, B_ONE, B_TAIL)
B_ORDER_HLL = (B_TINY, B_4M, B_EMPTY, B_ONE, B_HUGE, B_TAIL)  # the 16.9 M group immediately before the 30 reads


def layout_b(order=B_ORDER):
    """-> bases, offsets, group_offsets with the groups in `order` (fixed seed)"""
    if order not in _LAYOUT_B:
        groups = _b_groups()
        _LAYOUT_B[order] = assemble([groups[i] for i in order])
    return _LAYOUT_B[order]


B_CASES = {
    "prob3a_u64": params(A.ALGO_PROB3A, A.KMER64BIT, B_K, 64, A.SIG_U64),
    "super_f64": params(A.ALGO_SUPER, A.KMER64BIT, B_K, 64, A.SIG_F64),
    "optdens_f64": params(A.ALGO_OPTDENS, A.KMER64BIT, B_K, 9000, A.SIG_F64),
    "hll_u16": params(A.ALGO_HLL, A.KMER64BIT, B_K, 256, A.SIG_U16),
}
_ORACLE_B = {}  # case -> rows in B_ORDER


def oracle_rows_b(oracle, name):
    """the oracle rows of a case on layout B in B_ORDER, computed once (a few seconds of CPU per case)"""
    if name not in _ORACLE_B:
        bases, off, go = layout_b()
        _ORACLE_B[name] = oracle_rows(oracle, bases, off, go, B_CASES[name])
    return _ORACLE_B[name]


@gpu
@pytest.mark.parametrize("name", list(B_CASES))
def test_large_groups_oracle_and_all_seqs(ctx, oracle, name):
    p = B_CASES[name]
    bases, off, go = layout_b()
    got = np.asarray(ctx.sketch_groups(bases, off, go, p))
    assert got.shape == (6, p.sketch_size)
    assert_rows(got, own_rows(ctx, bases, off, go, p), name + " against kmu_sketch(ALL_SEQS) per group")
    assert_rows(got, oracle_rows_b(oracle, name), name + " against the oracle")


@gpu
def test_large_groups_hll_small_group_behind_the_largest(ctx, oracle):
    """K_low at size: by the time a workgroup turns to the 30 reads, many persistent workgroups have merged into the 16.9 M group's
    row; the 30 reads' registers must be their own"""
    p = B_CASES["hll_u16"]
    bases, off, go = layout_b(B_ORDER_HLL)
    got = np.asarray(ctx.sketch_groups(bases, off, go, p))
    want = oracle_rows_b(oracle, "hll_u16")[list(B_ORDER_HLL)]
    assert got[5].max() > 0
    assert_rows(got, want, "hll, reordered")


@gpu
def test_large_groups_device_packed(ctx, oracle):
    p = A.SketchParams.from_buffer_copy(B_CASES["prob3a_u64"])
    p.input_kind = A.INPUT_PACKED2
    bases, off, go = layout_b()
    data, poff = ctx.pack2b(bases, off)
    data = np.ascontiguousarray(np.concatenate([data, np.zeros(16, np.uint8)]))
    got = ctx.sketch_groups(to_dev(data), to_dev(off), to_dev(go), p, packed_offsets=to_dev(poff))
    assert got.is_cuda
    assert_rows(got, oracle_rows_b(oracle, "prob3a_u64"), "prob3a, device PACKED2")


# ---- no GPU: the layouts reach what the docstring says -------------------------------------------------------------------------
def test_layouts_reach_the_thresholds():
    for aa, ks in ((False, (12, 21)), (True, (7, 12))):
        bases, off, go = layout_a(aa)
        n_groups = len(go) - 1
        assert n_groups == 4100
        assert n_groups > 1024       # k_group_plan: blockDim.x, one trip of its group loop
        assert n_groups > 2 * 256    # k_grp_bounds: a grid of at most 2 x CUs workgroups, 256 CUs
        assert n_groups > 8 * 256    # k_grp_dens_finish: a grid of at most per_cu x CUs workgroups, per_cu <= 8, 256 CUs
        assert 1_300_000 < int(off[-1]) < 1_800_000
        sizes = np.diff(go.astype(np.int64))
        assert sorted(np.flatnonzero(sizes == 0).tolist()) == sorted(A_EMPTY)
        assert {1, 96, 4099} <= A_EMPTY and 0 not in A_EMPTY
        assert int(np.diff(off.astype(np.int64))[int(go[A_SHORT]):int(go[A_SHORT + 1])].max()) < min(ks)
        for k in ks:
            nk = group_kmers(off, go, k)
            multi = np.flatnonzero(nk > 4096)  # pmh_leaf_bits: more than 4 096 keys -> at least two leaves
            assert tuple(multi.tolist()) == A_MULTI == (7, 300, 511, 512, 800, 1023, 1025, 1500, 2047, 2049, 3000, 4098)
            assert nk[multi].min() >= 6000 and nk[multi].max() <= 20000
            assert nk[A_SHORT] == 0 and sizes[A_SHORT] == 5
        for lo, hi in ((0, 512), (512, 1024), (1025, 2048), (2049, 4100)):
            assert sum(lo <= g < hi for g in A_MULTI) >= 2
    bases, off, go = layout_b()
    assert len(go) - 1 == 6 and int(off[-1]) > 21_000_000 and int(off[-1]) < 24_000_000
    nk = group_kmers(off, go, B_K)
    # pmh_leaf_bits(n) >= 13 > GRP_LDS_BITS = 12 from 4097 x 4096 keys: the key-by-key branch of k_grp_hist / k_grp_scatter
    assert nk[B_HUGE] >= 16_781_312 + 100_000
    # pmh_leaf_bits(n) >= 11 from 4097 x 1024 keys: 2 048 leaves, two trips of k_grp_bounds' scan of 1 024
    assert 4_195_328 <= nk[B_4M] < 2 * 4_195_328
    # super_chunk_count(n) > 64 above 64 x 16 384 hashes: the second trip of k_grp_chunk_offsets
    assert nk[B_ONE] > 1_048_576 and go[B_ONE + 1] - go[B_ONE] == 1
    assert nk[B_TINY] == 30 and nk[B_EMPTY] == 0 and go[B_TAIL + 1] - go[B_TAIL] == 30
    lens = np.diff(off.astype(np.int64))[int(go[B_HUGE]):int(go[B_HUGE + 1])]
    assert lens.max() == 12_000_000 and int((lens >= 1_200_000).sum()) == 4 and int((lens <= 3000).sum()) == 200
    # the dens tile: total / (4 x walk_grid) above GD_TILE_MIN = 4 096; walk_grid is at most 5 workgroups x 256 CUs
    assert int(off[-1]) > 4096 * 4 * 5 * 256
    b2, o2, g2 = layout_b(B_ORDER_HLL)
    nk2 = group_kmers(o2, g2, B_K)
    assert nk2[4] == nk[B_HUGE] and g2[6] - g2[5] == 30 and int(o2[-1]) == int(off[-1])

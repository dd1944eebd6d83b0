"""-m "not gpu": the host side of seed chaining -- the symbol and its bindings, the constants and the record, refusals that need
no device, the index arithmetic of minimizer.seed_pairs / chain_hits on a stub context, and `reference_chains`: the contract of
kmu_seed_chains (include/kmu.h) as plain Python, which tests/test_gpu_chains.py compares the device against.  The reference is itself
checked here against a brute force over every chain of a small group, on positions drawn from tiny ranges so that ties and equal
x / y are everywhere, and on hand-made cases for each tie rule."""
import collections
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOOKBACK = 64  # (written out: test_constants_match_the_header compares it with the header and the binding)

# what the reference and Context.seed_chains read of a Minimizers record
Side = collections.namedtuple("Side", "pos read strand offsets")


def side(pos, read, strand=None, n_reads=None):
    read = np.array(read, np.uint32)
    n_reads = int(read.max()) + 1 if n_reads is None else n_reads
    return Side(np.array(pos, np.uint32), read, None if strand is None else np.array(strand, np.uint8), np.zeros(n_reads + 1, np.uint64))


def cost(g, span):
    return 0 if g == 0 else ((g * span) >> 7) + ((g.bit_length() - 1) >> 1)


def group_dp(xs, ys, span, max_gap, band):
    """f, start and n of every anchor of one group; xs, ys: Python ints in the group's (x, y) order"""
    n = len(xs)
    f, start, cnt = [span] * n, list(range(n)), [1] * n
    for i in range(n):
        best_t, best_j = span, -1
        for j in range(max(0, i - LOOKBACK), i):
            dx, dy = xs[i] - xs[j], ys[i] - ys[j]
            if not (0 < dx <= max_gap and 0 < dy <= max_gap) or abs(dx - dy) > band:
                continue
            t = f[j] + min(dx, dy, span) - cost(abs(dx - dy), span)
            if t > span and t >= best_t:  # strictly above a fresh start; j ascends, so >= leaves the largest j of the largest t
                best_t, best_j = t, j
        if best_j >= 0:
            f[i], start[i], cnt[i] = best_t, start[best_j], cnt[best_j] + 1
    return f, start, cnt


def reference_chains(pairs, q, db, span, max_gap, band, min_seeds=1, min_score=0, max_pos=0, upper=False):
    """the records of kmu_seed_chains as a structured array of A.CHAIN_DTYPE, by the text of include/kmu.h (max_pos is a promise
    about the input and changes no record: it is taken and not used)"""
    db = q if db is None else db
    pairs = np.asarray(pairs).astype(np.int64).reshape(-1, 2)
    ea, eb = pairs[:, 0], pairs[:, 1]
    zeros = np.zeros(pairs.shape[0], np.int64)
    sa = zeros if q.strand is None else np.asarray(q.strand).astype(np.int64)[ea]
    sb = zeros if db.strand is None else np.asarray(db.strand).astype(np.int64)[eb]
    ra, rb = np.asarray(q.read).astype(np.int64)[ea], np.asarray(db.read).astype(np.int64)[eb]
    x, pb, s = np.asarray(q.pos).astype(np.int64)[ea], np.asarray(db.pos).astype(np.int64)[eb], sa ^ sb
    groups = {}
    for t in zip(ra.tolist(), rb.tolist(), s.tolist(), x.tolist(), pb.tolist()):
        groups.setdefault(t[:3], []).append((t[3], -t[4] if t[2] else t[4]))
    best = {}  # read pair -> (f, s, i, record): the largest f, then s = 0, then the smallest i
    for (a, b, st) in sorted(groups):
        anchors = sorted(groups[(a, b, st)])
        xs, ys = [p[0] for p in anchors], [p[1] for p in anchors]
        f, start, cnt = group_dp(xs, ys, span, max_gap, band)
        i = max(range(len(f)), key=lambda t: (f[t], -t))
        if (a, b) in best and best[(a, b)][0] >= f[i]:  # (the groups of a read pair come s = 0 first)
            continue
        e, bg = i, start[i]
        pos_e, pos_b = abs(ys[e]), abs(ys[bg])
        best[(a, b)] = (f[i], (a, b, st, min(f[i], 2 ** 32 - 1), cnt[i], len(f), xs[bg], xs[e] + span,
                                pos_e if st else pos_b, (pos_b if st else pos_e) + span))
    rows = [rec for (a, b), (fi, rec) in sorted(best.items())
            if rec[3] >= min_score and rec[4] >= min_seeds and (not upper or a < b)]
    return np.array(rows, np.dtype(A.CHAIN_DTYPE)) if rows else np.zeros(0, np.dtype(A.CHAIN_DTYPE))


# ---- the reference against a brute force --------------------------------------------------------------------------------------
def brute_force_f(xs, ys, span, max_gap, band):
    """the best sum over every chain that ends at each anchor, chain by chain; shares no code with group_dp"""
    n = len(xs)

    def gain(j, i):  # None: j cannot come right before i
        if i - j > 64:
            return None
        dx, dy = xs[i] - xs[j], ys[i] - ys[j]
        if dx <= 0 or dy <= 0 or dx > max_gap or dy > max_gap:
            return None
        g = dx - dy if dx > dy else dy - dx
        if g > band:
            return None
        lg = 0
        while (2 << lg) <= g:
            lg += 1
        penalty = (g * span) // 128 + lg // 2 if g else 0
        return min(dx, dy, span) - penalty
    out = []
    for i in range(n):
        top = span
        for r in range(1, i + 1):
            for before in itertools.combinations(range(i), r):
                chain = list(before) + [i]
                steps = [gain(chain[t], chain[t + 1]) for t in range(len(chain) - 1)]
                if None not in steps:
                    top = max(top, span + sum(steps))
        out.append(top)
    return out


@pytest.mark.parametrize("hi,span,max_gap,band", [(4, 3, 3, 1), (8, 5, 6, 2), (8, 15, 8, 8), (40, 15, 25, 9), (3000, 21, 2000, 600)])
def test_reference_equals_the_brute_force_under_ties(hi, span, max_gap, band):
    rng = np.random.default_rng(hi + span)
    for rep in range(12):
        n = int(rng.integers(1, 11))
        anchors = sorted(zip(rng.integers(0, hi, n).tolist(), (rng.integers(0, hi, n) * rng.choice([1, -1])).tolist()))
        xs, ys = [a[0] for a in anchors], [a[1] for a in anchors]
        f, start, cnt = group_dp(xs, ys, span, max_gap, band)
        assert f == brute_force_f(xs, ys, span, max_gap, band), (xs, ys)
        for i in range(n):
            assert (start[i] == i) == (cnt[i] == 1) and (cnt[i] == 1) == (f[i] == span)  # a chained anchor is strictly above span
            assert start[i] <= i and 1 <= cnt[i] <= i - start[i] + 1


def test_cost_is_the_formula_of_the_header():
    assert [cost(g, 15) for g in (0, 1, 2, 3, 4, 7, 8, 9, 15, 16, 64, 1000)] == [0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 10, 121]
    assert cost(2 ** 31, 64) == 2 ** 30 + 15


# ---- each tie rule by hand ------------------------------------------------------------------------------------------------------
def one_pair(x, y, strand_b=None):
    """every (x[i], y[i]) an anchor of the read pair (0, 1): entries 0 .. n - 1 of q are read 0, of db read 1"""
    n = len(x)
    q = side(x, [0] * n, None if strand_b is None else [0] * n, 2)
    db = side(y, [1] * n, strand_b, 2)
    return np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32), q, db


def test_a_fresh_start_against_t_equal_to_span():
    # dx = 1, dy = 5: g = 4 costs 1 at span 15, min(dx, dy, span) = 1 -- t == span, not strictly larger: anchor 1 starts its own chain
    f, start, cnt = group_dp([0, 1], [0, 5], 15, 100, 100)
    assert (f, start, cnt) == ([15, 15], [0, 1], [1, 1])
    rec = reference_chains(*one_pair([0, 1], [0, 5]), 15, 100, 100)
    assert rec.tolist() == [(0, 1, 0, 15, 1, 2, 0, 15, 0, 15)]  # and of the two equal f the smallest i wins
    # one base further it pays: dx = 2, dy = 6
    assert group_dp([0, 2], [0, 6], 15, 100, 100) == ([15, 16], [0, 0], [1, 2])


def test_the_nearest_of_equal_predecessors():
    # anchors (0, 0) and (0, 1) cannot chain (dx = 0); (20, 21) gains 5 from either (g = 1 costs nothing): the larger j is taken
    f, start, cnt = group_dp([0, 0, 20], [0, 1, 21], 5, 100, 100)
    assert (f, start, cnt) == ([5, 5, 10], [0, 1, 1], [1, 1, 2])
    rec = reference_chains(*one_pair([0, 0, 20], [0, 1, 21]), 5, 100, 100)
    assert rec.tolist() == [(0, 1, 0, 10, 2, 3, 0, 25, 1, 26)]


def test_strand_0_before_strand_1():
    # the same chain on both strands: (10, 10) -> (30, 30) same strand, (10, 60) -> (30, 40) opposite (b runs backwards)
    x, y, sb = [10, 30, 10, 30], [10, 30, 60, 40], [0, 0, 1, 1]
    rec = reference_chains(*one_pair(x, y, sb), 15, 100, 100)
    assert rec.tolist() == [(0, 1, 0, 30, 2, 2, 10, 45, 10, 45)]
    # alone, the opposite strand reports b_start from its end anchor
    rec = reference_chains(*one_pair(x[2:], y[2:], sb[2:]), 15, 100, 100)
    assert rec.tolist() == [(0, 1, 1, 30, 2, 2, 10, 45, 40, 75)]
    # and a better chain on the opposite strand wins
    rec = reference_chains(*one_pair(x + [50], y + [20], sb + [1]), 15, 100, 100)
    assert rec.tolist() == [(0, 1, 1, 45, 3, 3, 10, 65, 20, 75)]


def test_the_smallest_i_of_equal_scores():
    # two chains of two seeds too far apart to join (max_gap 50): both end with f = 30, the first end wins
    rec = reference_chains(*one_pair([0, 20, 500, 520], [0, 20, 500, 520]), 15, 50, 10)
    assert rec.tolist() == [(0, 1, 0, 30, 2, 4, 0, 35, 0, 35)]


def test_filters_do_not_promote_a_runner_up():
    x, y, sb = [10, 30, 50, 10, 30], [10, 30, 50, 60, 40], [0, 0, 0, 1, 1]
    args = one_pair(x, y, sb)
    assert reference_chains(*args, 15, 100, 100).tolist() == [(0, 1, 0, 45, 3, 3, 10, 65, 10, 65)]
    assert reference_chains(*args, 15, 100, 100, min_seeds=3, min_score=45).shape == (1,)
    assert reference_chains(*args, 15, 100, 100, min_seeds=4).shape == (0,)   # the opposite strand's 2 seeds do not step in
    assert reference_chains(*args, 15, 100, 100, min_score=46).shape == (0,)
    assert reference_chains(*args, 15, 100, 100, upper=True).shape == (1,)
    pairs, q, db = args
    assert reference_chains(pairs[:, ::-1], db, q, 15, 100, 100, upper=True).shape == (0,)  # read_a = 1, read_b = 0


# ---- the symbol and its surroundings ------------------------------------------------------------------------------------------------
def test_symbol_and_bindings():
    """fails without the feature: the symbol is missing"""
    L = lib.load()
    assert "kmu_seed_chains" in lib.SYMBOLS and hasattr(L, "kmu_seed_chains")
    assert len(L.kmu_seed_chains.argtypes) == 18
    assert callable(getattr(lib.Context, "seed_chains"))
    assert callable(minimizer.chain_hits) and callable(minimizer.seed_pairs) and callable(minimizer.read_chains)


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    assert int(re.search(r"#define KMU_CHAIN_LOOKBACK (\d+)", txt).group(1)) == A.CHAIN_LOOKBACK == LOOKBACK
    assert int(re.search(r"#define KMU_CHAIN_UPPER (\d+)u", txt).group(1)) == A.CHAIN_UPPER == 1
    assert "int kmu_seed_chains(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs," in txt
    rec = re.search(r"typedef struct \{\s*/\* 40 bytes \*/(.*?)\} kmu_chain;", txt, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint32_t ([^;]+);", rec) for f in decl.split(",")]
    assert fields == [n for n, _ in A.CHAIN_DTYPE] == [n for n, _ in A.Chain._fields_]
    assert C.sizeof(A.Chain) == 40 and np.dtype(A.CHAIN_DTYPE).itemsize == 40
    par = re.search(r"typedef struct kmu_chain_params \{(.*?)\} kmu_chain_params;", txt, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", par) == [n for n, _ in A.ChainParams._fields_] and C.sizeof(A.ChainParams) == 28


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(4, np.uint32)
    p = A.ChainParams(15, 100, 100, 1, 0, 0, 0)
    n = C.c_uint64(77)
    a = arr.ctypes.data
    # no context: refused before anything is touched, whatever else is there
    assert L.kmu_seed_chains(None, a, 1, a, a, None, 4, 1, a, a, None, 4, 1, C.byref(p), A.MEM_HOST, None, 0, C.byref(n)) == A.E_BAD_ARG
    assert L.kmu_seed_chains(None, None, 1, None, None, None, 4, 1, None, None, None, 4, 1, None, A.MEM_HOST, None, 0, None) == A.E_BAD_ARG
    assert n.value == 77


# ---- seed_pairs and chain_hits on a stub context ----------------------------------------------------------------------------------
class _StubIndex:
    def __init__(self, ctx, hashes_db, n_keys, group_db):
        self.ctx = ctx
        ctx.created = (hashes_db, n_keys, group_db)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.closed = True

    def match(self, hashes_q, group_q=None, min_common=1, max_occ=0):
        self.ctx.matched = (hashes_q, group_q, min_common, max_occ)
        return self.ctx.pairs, np.zeros((self.ctx.pairs.shape[0], 3), np.uint32)


class _StubContext:
    def __init__(self, pairs):
        self.pairs = np.array(pairs, np.uint32).reshape(-1, 2)
        self.closed = False

    def anchor_index(self, hashes_db, n_keys=1, group_db=None):
        return _StubIndex(self, hashes_db, n_keys, group_db)

    def seed_chains(self, pairs, q, db, **kw):
        self.chained = (pairs, q, db, kw)
        return "records"


def _mini(hashes, pos, read, strand, k=21):
    return minimizer.Minimizers(np.array(hashes, np.uint64), np.array(pos, np.uint32), np.array(read, np.uint32),
                                None if strand is None else np.array(strand, np.uint8), np.zeros(max(read) + 2, np.uint64), k, 10,
                                A.FHASH_CANON_INVHASH)


def test_seed_pairs_and_chain_hits_index_arithmetic():
    q = _mini([5, 9, 5, 7], [3, 40, 11, 70000], [0, 0, 1, 2], [0, 1, 1, 0])
    hits = [[0, 2], [2, 0], [3, 1]]
    stub = _StubContext(hits)
    pairs = minimizer.seed_pairs(stub, q, max_occ=3)
    assert pairs is stub.pairs and pairs.tolist() == hits
    rows_db, n_keys, group_db = stub.created
    rows_q, group_q, min_common, max_occ = stub.matched
    assert rows_db.shape == (4, 1) and rows_q.shape == (4, 1) and rows_db[:, 0].tolist() == [5, 9, 5, 7]
    assert n_keys == 1 and group_db is q.read and group_q is q.read and (min_common, max_occ) == (1, 3) and stub.closed
    # seed_hits is the gather of exactly these pairs
    assert minimizer.seed_hits(_StubContext(hits), q, max_occ=3).tolist() == minimizer._gather6(pairs, q, q).tolist()
    db = _mini([7, 5], [8, 2], [0, 0], None)
    stub = _StubContext([[3, 0], [0, 1]])
    assert minimizer.seed_hits(stub, q, db).tolist() == minimizer._gather6(minimizer.seed_pairs(_StubContext([[3, 0], [0, 1]]), q, db), q, db).tolist()
    assert stub.created[2] is None and stub.matched[1] is None
    # chain_hits: the self-join reports each read pair once, the span is the k of the minimizers
    stub = _StubContext(hits)
    assert minimizer.chain_hits(stub, q, max_occ=2) == "records"
    pairs, cq, cdb, kw = stub.chained
    assert pairs is stub.pairs and cq is q and cdb is None and stub.matched[3] == 2 and stub.created[2] is q.read
    assert kw == dict(span=21, max_gap=5000, band=500, min_seeds=3, min_score=0, upper=True)
    stub = _StubContext([[3, 0]])
    minimizer.chain_hits(stub, q, db, max_gap=70, band=9, min_seeds=1, min_score=4)
    pairs, cq, cdb, kw = stub.chained
    assert cq is q and cdb is db and stub.created[2] is None
    assert kw == dict(span=21, max_gap=70, band=9, min_seeds=1, min_score=4, upper=False)
    minimizer.chain_hits(stub, q, db, upper=True)
    assert stub.chained[3]["upper"] is True

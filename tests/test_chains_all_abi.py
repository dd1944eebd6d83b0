"""-m "not gpu": the host side of kmu_seed_chains_all and kmu_chain_rank -- the symbols and their bindings, the constants and the
records, refusals that need no device, `chain_mapq` and the PAF columns, and the two references the GPU tests compare the device
against: `reference_chains_all` and `reference_rank`, the contracts of include/kmu.h as plain Python.  The chains are taken from the
`best` definition; a greedy back-tracking that shares no code with it (ends by descending f, walk back to the first used anchor)
must give the same chains on groups whose coordinates are so small that ties are everywhere, and the first chain of every read
pair must be the record of `reference_chains`."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_chains_abi import LOOKBACK, Side, cost, group_dp, one_pair, reference_chains, side  # noqa: E402,F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = np.dtype(A.CHAIN_DTYPE)
RANK = np.dtype(A.CHAIN_RANK_DTYPE)
TIES = [(3, 4, 2), (2, 7, 7), (64, 3, 0)]  # (span, max_gap, band) of test_ties_everywhere


# ---- reference_chains_all -------------------------------------------------------------------------------------------------------
def group_dp_pred(xs, ys, span, max_gap, band):
    """f and pred (None: none) of every anchor of one group, by the header: strictly above span, the largest j of the largest t"""
    n = len(xs)
    f, pred = [span] * n, [None] * n
    for i in range(n):
        for j in range(max(0, i - LOOKBACK), i):
            dx, dy = xs[i] - xs[j], ys[i] - ys[j]
            if dx <= 0 or dy <= 0 or dx > max_gap or dy > max_gap or abs(dx - dy) > band:
                continue
            t = f[j] + min(dx, dy, span) - cost(abs(dx - dy), span)
            if t > span and (pred[i] is None or t >= f[i]):
                f[i], pred[i] = t, j
    assert f == group_dp(xs, ys, span, max_gap, band)[0]
    return f, pred


def best_of(f, pred):
    """best(v): among v and every anchor whose pred path reaches v the one with the largest f, the smallest index on a tie"""
    n = len(f)
    best = list(range(n))
    for d in range(n):
        v = pred[d]
        while v is not None:
            if (f[d], -d) > (f[best[v]], -best[v]):
                best[v] = d
            v = pred[v]
    return best


def group_chains(f, pred):
    """the chains of one group as (e, b, n, unclamped score), by ascending e"""
    best = best_of(f, pred)
    out = []
    for e in range(len(f)):
        if best[e] != e:
            continue
        members = [v for v in range(len(f)) if best[v] == e]
        b = members[0]
        walk = [e]  # the members are a path that ends in e
        while walk[-1] != b:
            walk.append(pred[walk[-1]])
        assert sorted(walk) == members
        p = pred[b]
        assert p is None or best[p] != e
        out.append((e, b, len(members), f[e] - (f[p] if p is not None else 0)))
    return out


def greedy_chains(f, pred):
    """back-tracking: the ends by (-f, i); each walks back until it reaches an anchor that is already used"""
    used, out = [False] * len(f), []
    for e in sorted(range(len(f)), key=lambda i: (-f[i], i)):
        if used[e]:
            continue
        v, n, b = e, 0, e
        while v is not None and not used[v]:
            used[v] = True
            n, b, v = n + 1, v, pred[v]
        out.append((e, b, n, f[e] - (f[v] if v is not None else 0)))
    return sorted(out)


def all_groups(pairs, q, db):
    """{(read_a, read_b, strand): sorted [(x, y)]} of the pairs"""
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
    return {key: sorted(v) for key, v in groups.items()}


def reference_chains_all(pairs, q, db, span, max_gap, band, min_seeds=1, min_score=0, max_pos=0, upper=False, details=False):
    """the records of kmu_seed_chains_all as a structured array of A.CHAIN_DTYPE, by the text of include/kmu.h; details=True:
    (records, [(e, unclamped score)]) of the same chains (max_pos is a promise about the input and changes no record)"""
    rows, extra = [], []
    groups = all_groups(pairs, q, db)
    for (a, b, st) in sorted(groups):
        xs, ys = [p[0] for p in groups[(a, b, st)]], [p[1] for p in groups[(a, b, st)]]
        f, pred = group_dp_pred(xs, ys, span, max_gap, band)
        for e, bg, n, raw in group_chains(f, pred):
            score = min(max(raw, 0), 2 ** 32 - 1)
            if score < min_score or n < min_seeds or (upper and not a < b):
                continue
            pos_e, pos_b = abs(ys[e]), abs(ys[bg])
            rows.append((a, b, st, score, n, len(f), xs[bg], xs[e] + span, pos_e if st else pos_b, (pos_b if st else pos_e) + span))
            extra.append((e, raw))
    rec = np.array(rows, REC) if rows else np.zeros(0, REC)
    return (rec, extra) if details else rec


def small_batch(seed, n_pairs=1500, nq=60, ndb=50, hi=8):
    rng = np.random.default_rng(seed)
    q = side(rng.integers(0, hi, nq), rng.integers(0, 4, nq), rng.integers(0, 2, nq), 4)
    db = side(rng.integers(0, hi, ndb), rng.integers(0, 3, ndb), rng.integers(0, 2, ndb), 3)
    return np.stack([rng.integers(0, nq, n_pairs), rng.integers(0, ndb, n_pairs)], axis=1).astype(np.uint32), q, db


@pytest.mark.parametrize("span,max_gap,band", TIES)
def test_best_definition_equals_greedy_back_tracking(span, max_gap, band):
    rng = np.random.default_rng(span)
    forks = 0
    for rep in range(60):
        n = int(rng.integers(1, 90))
        anchors = sorted(zip(rng.integers(0, 8, n).tolist(), (rng.integers(0, 8, n) * rng.choice([1, -1])).tolist()))
        xs, ys = [a[0] for a in anchors], [a[1] for a in anchors]
        f, pred = group_dp_pred(xs, ys, span, max_gap, band)
        assert all(p is None or p < i for i, p in enumerate(pred))
        chains = group_chains(f, pred)
        assert chains == greedy_chains(f, pred), (xs, ys)
        assert sum(c[2] for c in chains) == n  # every anchor is in exactly one chain
        forks += sum(1 for c in chains if pred[c[1]] is not None)
    assert span == 64 or forks > 0  # chains that branch off another one were there


@pytest.mark.parametrize("span,max_gap,band", TIES + [(15, 60, 20)])
def test_first_chain_of_a_read_pair_is_the_record_of_seed_chains(span, max_gap, band):
    pairs, q, db = small_batch(span) if span != 15 else small_batch(5, 3000, 400, 400, 300)
    rec, extra = reference_chains_all(pairs, q, db, span, max_gap, band, details=True)
    first = {}
    for r, (e, raw) in zip(rec.tolist(), extra):
        key = (-raw, r[2], e)
        if (r[0], r[1]) not in first or key < first[(r[0], r[1])][0]:
            first[(r[0], r[1])] = (key, r)
    want = reference_chains(pairs, q, db, span, max_gap, band)
    assert [first[k][1] for k in sorted(first)] == want.tolist() and want.shape[0] > 5


def test_hand_made_fork():
    # (0, 0) -> (20, 20) -> (40, 40) and a branch (0, 0) -> (20, 24): g = 4 costs 1, f = 15 + 15 - 1 = 29 against 30 and 45
    pairs, q, db = one_pair([0, 20, 20, 40], [0, 20, 24, 40])
    rec = reference_chains_all(pairs, q, db, 15, 100, 10)
    # the branch leaves anchor 0, which belongs to the main chain: score 29 - f(0) = 14, one seed, starts at its own anchor
    assert rec.tolist() == [(0, 1, 0, 14, 1, 4, 20, 35, 24, 39), (0, 1, 0, 45, 3, 4, 0, 55, 0, 55)]
    assert reference_chains_all(pairs, q, db, 15, 100, 10, min_score=15).tolist() == [(0, 1, 0, 45, 3, 4, 0, 55, 0, 55)]
    assert reference_chains_all(pairs, q, db, 15, 100, 10, min_seeds=2).shape == (1,)  # the branch's anchor goes nowhere
    assert reference_chains_all(pairs[:, ::-1], db, q, 15, 100, 10, upper=True).shape == (0,)
    # both strands with the same chain: two records, strand 0 first
    both = one_pair([10, 30, 10, 30], [10, 30, 60, 40], [0, 0, 1, 1])
    assert reference_chains_all(*both, 15, 100, 100).tolist() == [(0, 1, 0, 30, 2, 2, 10, 45, 10, 45), (0, 1, 1, 30, 2, 2, 10, 45, 40, 75)]


def test_a_branch_below_its_parent_scores_zero():
    # one path whose last step loses: g = 300 costs (300 * 64 >> 7) + (8 >> 1) = 154 against a gain of 64, t = 192 - 90 = 102 > span
    f, pred = group_dp_pred([0, 100, 200, 300], [0, 100, 200, 600], 64, 1000, 1000)
    assert (f, pred) == ([64, 128, 192, 102], [None, 0, 1, 2])
    assert group_chains(f, pred) == [(2, 0, 3, 192), (3, 3, 1, -90)]  # anchor 2 is its own best: the path is cut behind it
    # a fork: the main chain goes on to (60, 60); (60, 260) leaves anchor 2 with g = 200, cost 23 + 3 against a gain of 15
    pairs, q, db = fork_below_its_parent()
    rec = reference_chains_all(pairs, q, db, 15, 1000, 1000)
    assert rec.tolist() == [(0, 1, 0, 60, 4, 5, 0, 75, 0, 75), (0, 1, 0, 0, 1, 5, 60, 75, 260, 275)]
    assert reference_chains_all(pairs, q, db, 15, 1000, 1000, min_score=1).shape == (1,)


def fork_below_its_parent():
    return one_pair([0, 20, 40, 60, 60], [0, 20, 40, 60, 260])


# ---- reference_rank -------------------------------------------------------------------------------------------------------------
def reference_rank(chains, n_reads_q, mask_permille=500):
    """the records of kmu_chain_rank as a structured array of A.CHAIN_RANK_DTYPE, by the text of include/kmu.h; ValueError where
    the call answers KMU_E_UNSUPPORTED"""
    c = np.asarray(chains)
    ra, score = c["read_a"].astype(np.int64).tolist(), c["score"].astype(np.int64).tolist()
    s, e = c["a_start"].astype(np.int64).tolist(), c["a_end"].astype(np.int64).tolist()
    n = len(ra)
    if any(ra[i] < ra[i - 1] for i in range(1, n)) or any(r >= n_reads_q for r in ra) or any(s[i] > e[i] for i in range(n)):
        raise ValueError("unsupported")
    out = np.zeros(n, RANK)
    by_read = {}
    for i in range(n):
        by_read.setdefault(ra[i], []).append(i)
    for idx in by_read.values():
        primaries = []
        for rank, i in enumerate(sorted(idx, key=lambda i: (-score[i], i))):
            parent = i
            for pr in primaries:
                ov = max(0, min(e[i], e[pr]) - max(s[i], s[pr]))
                if ov > 0 and ov * 1000 >= mask_permille * min(e[i] - s[i], e[pr] - s[pr]):
                    parent = pr
                    break
            out[i]["rank"], out[i]["parent"] = rank, parent
            if parent == i:
                primaries.append(i)
            else:
                if out[parent]["n_sub"] == 0:
                    out[parent]["sub_score"] = score[i]
                out[parent]["n_sub"] += 1
    return out


def chain_records(rows):
    """rows of (read_a, score, a_start, a_end) as chain records"""
    rec = np.zeros(len(rows), REC)
    for i, (ra, score, s, e) in enumerate(rows):
        rec[i] = (ra, 0, 0, score, 3, 3, s, e, s, e)
    return rec


def test_reference_rank_by_hand():
    # the mask edge: the shorter chain has 200 bases; at 500 permille an overlap of 100 is enough (100 * 1000 == 500 * 200), 99 is not
    rec = chain_records([(0, 90, 0, 1000), (0, 50, 900, 1100), (0, 40, 2000, 2200), (0, 30, 2101, 2301)])
    assert reference_rank(rec, 1).tolist() == [(0, 0, 50, 1), (1, 0, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0)]
    rec["a_start"][3], rec["a_end"][3] = 2100, 2300
    assert reference_rank(rec, 1).tolist() == [(0, 0, 50, 1), (1, 0, 0, 0), (2, 2, 30, 1), (3, 2, 0, 0)]
    assert reference_rank(rec, 1, 501).tolist() == [(0, 0, 0, 0), (1, 1, 0, 0), (2, 2, 0, 0), (3, 3, 0, 0)]
    # equal scores fall back to the input index
    rec = chain_records([(0, 7, 0, 100), (0, 9, 50, 150), (0, 9, 60, 160), (0, 7, 500, 600)])
    assert reference_rank(rec, 1)["rank"].tolist() == [2, 0, 1, 3]
    assert reference_rank(rec, 1)["parent"].tolist() == [1, 1, 1, 3]
    # a secondary never becomes a parent: chain 2 overlaps the secondary 1 only and stays primary
    rec = chain_records([(0, 90, 0, 1000), (0, 50, 600, 1300), (0, 40, 1100, 1400)])
    assert reference_rank(rec, 1).tolist() == [(0, 0, 50, 1), (1, 0, 0, 0), (2, 2, 0, 0)]
    # reads rank apart; sub_score is the best secondary, n_sub counts them; mask 0: any overlap; an empty interval overlaps nothing
    rec = chain_records([(0, 10, 0, 100), (0, 20, 0, 100), (0, 5, 0, 100), (2, 10, 0, 100), (2, 9, 99, 300), (2, 8, 100, 300), (2, 7, 50, 50)])
    assert reference_rank(rec, 3, 0).tolist() == [(1, 1, 0, 0), (0, 1, 10, 2), (2, 1, 0, 0), (0, 3, 9, 1), (1, 3, 0, 0), (2, 5, 0, 0), (3, 6, 0, 0)]
    for bad in (chain_records([(1, 5, 0, 9), (0, 5, 0, 9)]), chain_records([(3, 5, 0, 9)]), chain_records([(0, 5, 10, 9)])):
        with pytest.raises(ValueError):
            reference_rank(bad, 3)
    assert reference_rank(rec[:0], 3).shape == (0,)


# ---- mapping quality and PAF ----------------------------------------------------------------------------------------------------
def test_chain_mapq_by_hand():
    rec = chain_records([(0, 100, 0, 10), (0, 100, 0, 10), (0, 30, 0, 10), (0, 50, 0, 10), (0, 0, 0, 10), (0, 100, 0, 10)])
    rec["n_seeds"] = [10, 5, 3, 40, 9, 10]
    rank = np.zeros(6, RANK)
    rank["parent"] = [0, 1, 2, 3, 4, 0]  # the last one is a secondary
    rank["sub_score"] = [0, 50, 15, 40, 0, 0]
    # 40 * ln(100) = 184.2 -> 60; 40 * .5 * .5 * 4.605 = 46.05; 40 * .5 * .3 * 3.401 = 20.4; 40 * .2 * 3.912 = 31.3; score 0; secondary
    assert minimizer.chain_mapq(rec, rank).tolist() == [60, 46, 20, 31, 0, 0]


def test_paf_lines_with_a_rank_array():
    rec = chain_records([(0, 100, 5, 500), (0, 50, 100, 300)])
    rec["read_b"], rec["n_seeds"] = [1, 0], [5, 4]
    aln = np.array([(7, 480, 30, A.ALN_DONE | A.ALN_EXACT), (0, 0, 3000, 0)], np.dtype(A.CHAIN_ALN_DTYPE))
    rank = reference_rank(rec, 1)
    assert rank.tolist() == [(0, 0, 50, 1), (1, 0, 0, 0)]
    names, off = ["r0"], [0, 900]
    names_db, off_db = ["c0", "c1"], [0, 4000, 9000]
    plain = minimizer.paf_lines(rec, aln, names, off, names_db, off_db)
    assert plain[0] == "r0\t900\t5\t500\t+\tc1\t5000\t5\t500\t480\t487\t255\tNM:i:7\ts1:i:100\tcm:i:5"
    got = minimizer.paf_lines(rec, aln, names, off, names_db, off_db, rank=rank)
    assert got[0] == "r0\t900\t5\t500\t+\tc1\t5000\t5\t500\t480\t487\t46\tNM:i:7\ts1:i:100\tcm:i:5\ttp:A:P\ts2:i:50"
    assert got[1] == "r0\t900\t100\t300\t+\tc0\t4000\t100\t300\t0\t200\t0\ts1:i:50\tcm:i:4\ttp:A:S\ts2:i:0"


# ---- the symbols and their surroundings -------------------------------------------------------------------------------------------
def test_symbols_and_bindings():
    """fails without the feature: the symbols are missing"""
    L = lib.load()
    for name in ("kmu_seed_chains_all", "kmu_chain_rank"):
        assert name in lib.SYMBOLS and hasattr(L, name), name
    assert len(L.kmu_seed_chains_all.argtypes) == 18 and L.kmu_seed_chains_all.argtypes == L.kmu_seed_chains.argtypes
    assert len(L.kmu_chain_rank.argtypes) == 7
    assert callable(lib.Context.seed_chains_all) and callable(lib.Context.chain_rank)
    for f in (minimizer.rank_chains, minimizer.chain_mapq, minimizer.map_reads):
        assert callable(f)
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        txt = open(os.path.join(ROOT, doc)).read()
        assert "kmu_seed_chains_all" in txt and "kmu_chain_rank" in txt, doc


def test_constants_and_struct_sizes_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    assert "int kmu_seed_chains_all(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs," in txt
    assert "int kmu_chain_rank(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, uint32_t n_reads_q," in txt
    rec = re.search(r"typedef struct \{\s*uint32_t ([^;]+);\s*\} kmu_chain_rank_rec;\s*/\* 16 bytes \*/", txt).group(1)
    fields = [f.strip() for f in rec.split(",")]
    assert fields == [n for n, _ in A.CHAIN_RANK_DTYPE] == [n for n, _ in A.ChainRank._fields_]
    assert C.sizeof(A.ChainRank) == 16 and RANK.itemsize == 16
    par = re.search(r"typedef struct kmu_rank_params \{(.*?)\} kmu_rank_params;", txt, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", par) == [n for n, _ in A.RankParams._fields_] and C.sizeof(A.RankParams) == 8
    assert int(re.search(r"#define KMU_CHAIN_LOOKBACK (\d+)", txt).group(1)) == A.CHAIN_LOOKBACK == LOOKBACK


def test_refusals_that_need_no_device():
    L = lib.load()
    arr = np.zeros(4, np.uint32)
    p = A.ChainParams(15, 100, 100, 1, 0, 0, 0)
    n = C.c_uint64(77)
    a = arr.ctypes.data
    bad = A.E_BAD_ARG
    assert L.kmu_seed_chains_all(None, a, 1, a, a, None, 4, 1, a, a, None, 4, 1, C.byref(p), A.MEM_HOST, None, 0, C.byref(n)) == bad
    assert L.kmu_seed_chains_all(None, None, 1, None, None, None, 4, 1, None, None, None, 4, 1, None, A.MEM_HOST, None, 0, None) == bad
    assert n.value == 77
    chains, out = np.zeros(2, REC), np.full(2, 9, np.uint32).astype(RANK)
    rp = A.RankParams(500, 0)
    assert L.kmu_chain_rank(None, chains.ctypes.data, 2, 1, C.byref(rp), A.MEM_HOST, out.ctypes.data) == bad
    assert L.kmu_chain_rank(None, None, 0, 1, None, A.MEM_HOST, None) == bad
    assert out.tolist() == [(9, 9, 9, 9)] * 2


# ---- chain_hits(all=True) on a stub context ---------------------------------------------------------------------------------------
def test_chain_hits_selects_the_entry():
    from test_chains_abi import _mini, _StubContext

    class Stub(_StubContext):
        def seed_chains_all(self, pairs, q, db, **kw):
            self.chained_all = (pairs, q, db, kw)
            return "all records"

        def chain_rank(self, chains, n_reads_q, mask_permille=500):
            return ("rank", chains, n_reads_q, mask_permille)

    q = _mini([5, 9, 5, 7], [3, 40, 11, 70000], [0, 0, 1, 2], [0, 1, 1, 0])
    stub = Stub([[0, 2], [2, 0]])
    assert minimizer.chain_hits(stub, q, max_occ=2) == "records" and not hasattr(stub, "chained_all")
    assert minimizer.chain_hits(stub, q, max_occ=2, all=True) == "all records"
    pairs, cq, cdb, kw = stub.chained_all
    assert pairs is stub.pairs and cq is q and cdb is None
    assert kw == dict(span=21, max_gap=5000, band=500, min_seeds=3, min_score=0, upper=True)
    assert minimizer.rank_chains(stub, "c", 3, mask_permille=100) == ("rank", "c", 3, 100)

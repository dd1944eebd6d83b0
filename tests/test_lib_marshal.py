"""-m "not gpu": what the wrappers of kmerutils_amd/lib.py hand to the C ABI, on a recording stand-in for the library -- no device
and no libkmu.so.  Every call is written down as (name, arguments): integers and parameter structs by value, and every pointer as
None, the name of the input it is the base address of, "retN" (the base address of the N-th returned array) or "#k" (another
non-null address, numbered by first appearance over the calls of one wrapper: one placeholder shared by two arguments shows as
the same number, two placeholders as two).  The numbers are stable because the recorded pointers keep their arrays alive (numpy's
ctypes.data_as holds a reference): without that a placeholder freed after one call could give its address to the next one, and
two numbers would collapse into one.  Host (numpy) inputs only: the device branches run in the -m gpu tests."""
import ctypes as C
import types

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib

H_CTX, H_OBJ = 0x1000, 0x2000
REF = "&"  # a byref() out-parameter that is no parameter struct


class Recorder:
    """stands where Context.L does: any attribute is a function that notes (name, args), stores `answers[name]` -- {argument
    index: value} -- through the byref arguments named there, and returns 0"""

    def __init__(self, answers):
        self.calls, self.answers = [], answers

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, args))
            for at, value in self.answers.get(name, {}).items():
                args[at]._obj.value = value
            return 0
        return fn


def context(answers=None):
    ctx = object.__new__(lib.Context)
    ctx.h, ctx.device_id, ctx._stream, ctx.L = C.c_void_p(H_CTX), 0, 0, Recorder(answers or {})
    return ctx


def handle(cls, ctx, **attrs):
    obj = object.__new__(cls)
    obj.ctx, obj.L, obj.h = ctx, ctx.L, C.c_void_p(H_OBJ)
    for k, v in attrs.items():
        setattr(obj, k, v)
    ctx.kept = getattr(ctx, "kept", []) + [obj]  # (alive as long as the context: no destroy call from a collected temporary)
    return obj


def drive(call, inputs=None, answers=None):
    """call(ctx) on a fresh stand-in context; (what it returned as a tuple, the calls it made in the notation above)"""
    ctx = context(answers)
    ret = call(ctx)
    ret = tuple(ret) if isinstance(ret, (tuple, list)) else (ret,)
    names = {H_CTX: "ctx", H_OBJ: "h"}
    for k, x in (inputs or {}).items():
        if isinstance(x, np.ndarray) and x.size:
            names.setdefault(x.ctypes.data, k)
    for i, x in enumerate(ret):
        if isinstance(x, np.ndarray):
            names.setdefault(x.ctypes.data, "ret%d" % i)
    others, rows = {}, []
    for name, args in ctx.L.calls:
        row = [name]
        for a in args:
            if a is None or isinstance(a, int):
                row.append(a)
            elif isinstance(a, C.c_void_p):
                v = a.value
                row.append(None if v is None else names[v] if v in names else others.setdefault(v, "#%d" % len(others)))
            elif isinstance(a._obj, C.Structure) and type(a._obj).__name__.endswith("Params"):
                row.append((type(a._obj).__name__,) + tuple(getattr(a._obj, f[0]) for f in a._obj._fields_))
            else:
                row.append(REF)
        rows.append(tuple(row))
    ctx.h = None  # (nothing to destroy)
    return ret, rows


def same_calls(got, want):
    assert len(got) == len(want), [r[0] for r in got]
    for g, w in zip(got, want):
        assert g == tuple(w), "\n got  %r\n want %r" % (g, tuple(w))


def shapes(ret, *want):
    """every returned array by (dtype, shape); None for a None"""
    assert len(ret) == len(want)
    for x, w in zip(ret, want):
        if w is None:
            assert x is None
        else:
            assert isinstance(x, np.ndarray) and x.dtype == np.dtype(w[0]) and x.shape == tuple(w[1]), (x.dtype, x.shape, w)


def raises(msg, call):
    with pytest.raises(ValueError) as e:
        call(context())
    assert str(e.value) == msg


def u8(n):
    return np.frombuffer((b"ACGTACGTACGT" * 4)[:n], np.uint8).copy()


def recs(n, dtype):
    return np.zeros(n, np.dtype(dtype))


CHAIN, ALN = np.dtype(A.CHAIN_DTYPE), np.dtype(A.CHAIN_ALN_DTYPE)
OFFSET_FORMS = (lambda x: list(x), lambda x: np.array(x, np.int64), lambda x: np.array(x, np.uint64))


# ---- signature comparison ----
def test_sig_equal_matrix():
    a, b = np.ones((2, 4), np.uint32), np.ones((3, 4), np.uint32)
    ret, calls = drive(lambda c: c.sig_equal_matrix(a, b), dict(a=a, b=b))
    same_calls(calls, [("kmu_sig_equal_matrix", "ctx", "a", 2, "b", 3, 4, A.SIG_U32, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint16, (2, 3)))
    e = np.ones((0, 4), np.uint32)
    ret, calls = drive(lambda c: c.sig_equal_matrix(e, b), dict(a=e, b=b))
    same_calls(calls, [("kmu_sig_equal_matrix", "ctx", "ret0", 0, "b", 3, 4, A.SIG_U32, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint16, (0, 3)))
    ret, calls = drive(lambda c: c.sig_equal_matrix(a, e), dict(a=a, b=e))
    same_calls(calls, [("kmu_sig_equal_matrix", "ctx", "a", 2, "ret0", 0, 4, A.SIG_U32, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint16, (2, 0)))


def test_sig_knn():
    q, db, gq = np.ones((2, 4), np.uint64), np.ones((3, 4), np.uint64), np.zeros(2, np.uint32)
    ret, calls = drive(lambda c: c.sig_knn(q, db, 2, group_q=gq), dict(q=q, db=db, gq=gq))
    same_calls(calls, [("kmu_sig_knn", "ctx", "q", 2, "db", 3, 4, A.SIG_U64, 2, "gq", None, A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint32, (2, 2)), (np.uint16, (2, 2)))
    e = np.ones((0, 4), np.uint64)
    ret, calls = drive(lambda c: c.sig_knn(e, e, 2), dict(q=e, db=e))
    same_calls(calls, [("kmu_sig_knn", "ctx", "ret0", 0, "ret0", 0, 4, A.SIG_U64, 2, None, None, A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint32, (0, 2)), (np.uint16, (0, 2)))
    raises("query and database signatures differ in type or sketch size", lambda c: c.sig_knn(q, np.ones((3, 5), np.uint64), 2))


# ---- anchors ----
@pytest.mark.parametrize("total", [0, 3])
def test_anchor_match(total):
    q, db, gdb = np.ones((2, 4), np.uint64), np.ones((3, 4), np.uint64), np.zeros(3, np.uint32)
    ret, calls = drive(lambda c: c.anchor_match(q, db, n_keys=2, min_common=3, group_db=gdb), dict(q=q, db=db, gdb=gdb),
                       {"kmu_anchor_match": {-1: total}})
    lead = ("kmu_anchor_match", "ctx", "q", 2, "db", 3, 4, 2, 3, None, "gdb", A.MEM_HOST)
    same_calls(calls, [lead + (None, None, 0, REF)] + ([lead + ("ret0", "ret1", 3, REF)] if total else []))
    shapes(ret, (np.uint32, (total, 2)), (np.uint32, (total, 3)))


def test_anchor_match_empty_sides():
    e, db = np.ones((0, 4), np.uint64), np.ones((3, 4), np.uint64)
    ret, calls = drive(lambda c: c.anchor_match(e, db), dict(q=e, db=db), {"kmu_anchor_match": {-1: 3}})
    lead = ("kmu_anchor_match", "ctx", "#0", 0, "db", 3, 4, 1, 1, None, None, A.MEM_HOST)
    same_calls(calls, [lead + (None, None, 0, REF), lead + ("ret0", "ret1", 3, REF)])
    ret, calls = drive(lambda c: c.anchor_match(e, e), dict(q=e, db=e))
    same_calls(calls, [("kmu_anchor_match", "ctx", "#0", 0, "#0", 0, 4, 1, 1, None, None, A.MEM_HOST, None, None, 0, REF)])
    raises("query and database rows differ in length", lambda c: c.anchor_match(db, np.ones((3, 5), np.uint64)))


def test_count_then_write():
    x = np.ones(2, np.uint32)
    ctx = context()
    calls = []

    def fn(*args):
        calls.append(args)
        args[-1]._obj.value = 3
        return 0
    pairs, dist = ctx._count_then_write(fn, (7, 8), x)
    assert [a[:2] + a[4:5] for a in calls] == [(7, 8, 0), (7, 8, 3)] and calls[0][2:4] == (None, None)
    assert (calls[1][2].value, calls[1][3].value) == (pairs.ctypes.data, dist.ctypes.data)
    shapes((pairs, dist), (np.uint32, (3, 2)), (np.uint32, (3, 3)))
    ctx.h = None


def test_anchor_index():
    db, gdb, q = np.ones((3, 4), np.uint64), np.zeros(3, np.uint32), np.ones((2, 4), np.uint64)
    answers = {"kmu_anchor_index_create": {-1: H_OBJ}, "kmu_anchor_index_match": {-1: 3}}

    def run(c):
        with lib.AnchorIndex(c, db, 2, gdb) as ix:
            assert ix.m == 4 and ix.h.value == H_OBJ
            got = ix.match(q, min_common=2, max_occ=5)
        assert ix.h is None
        ix.close()  # (closing twice is silent)
        return got
    ret, calls = drive(run, dict(db=db, gdb=gdb, q=q), answers)
    lead = ("kmu_anchor_index_match", "h", "q", 2, None, 2, 5, A.MEM_HOST)
    same_calls(calls, [("kmu_anchor_index_create", "ctx", "db", 3, 4, 2, "gdb", A.MEM_HOST, REF), lead + (None, None, 0, REF),
                       lead + ("ret0", "ret1", 3, REF), ("kmu_anchor_index_destroy", "h")])
    shapes(ret, (np.uint32, (3, 2)), (np.uint32, (3, 3)))
    e = np.ones((0, 4), np.uint64)

    def run_empty(c):
        ix = lib.AnchorIndex(c, e)
        got = ix.match(e)
        c.h = None
        ix.close()  # (after the context: silent, and nothing is destroyed)
        c.h = C.c_void_p(H_CTX)
        return got
    answers["kmu_anchor_index_match"] = {-1: 0}
    ret, calls = drive(run_empty, dict(db=e), answers)
    same_calls(calls, [("kmu_anchor_index_create", "ctx", "#0", 0, 4, 1, None, A.MEM_HOST, REF),
                       ("kmu_anchor_index_match", "h", "#1", 0, None, 1, 0, A.MEM_HOST, None, None, 0, REF)])
    shapes(ret, (np.uint32, (0, 2)), (np.uint32, (0, 3)))
    with pytest.raises(ValueError) as err:
        handle(lib.AnchorIndex, context(), m=4).match(np.ones((2, 5), np.uint64))
    assert str(err.value) == "query rows and the index's rows differ in length"


@pytest.mark.parametrize("total", [0, 3])
@pytest.mark.parametrize("form", range(3))
def test_anchor_overlaps(total, form):
    pairs, dist = np.ones((3, 2), np.uint32), np.ones((3, 3), np.uint32)
    rq, rdb = OFFSET_FORMS[form]([0, 2, 5]), OFFSET_FORMS[form]([0, 1, 2, 3])
    answers = {"kmu_anchor_overlaps": {-1: total}}
    ret, calls = drive(lambda c: c.anchor_overlaps(pairs, dist, rq, band=4, min_score=2, upper=True), dict(pairs=pairs, dist=dist), answers)
    lead = ("kmu_anchor_overlaps", "ctx", "pairs", "dist", 3, "#0", 2, "#0", 2, 2, 4, 2, A.OVL_UPPER, A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    shapes(ret, (A.OVERLAP_DTYPE, (total,)))
    ret, calls = drive(lambda c: c.anchor_overlaps(pairs, None, rq, rdb, strands=1), dict(pairs=pairs), answers)
    lead = ("kmu_anchor_overlaps", "ctx", "pairs", None, 3, "#0", 2, "#1", 3, 1, 1, 1, 0, A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    e = np.ones((0, 2), np.uint32)
    ret, calls = drive(lambda c: c.anchor_overlaps(e, None, rq, rq), dict(pairs=e), answers)
    lead = ("kmu_anchor_overlaps", "ctx", "#0", None, 0, "#1", 2, "#1", 2, 2, 1, 1, 0, A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))


def minimizers(n, n_reads=2, strand=True):
    return types.SimpleNamespace(pos=np.ones(n, np.uint32), read=np.zeros(n, np.uint32), strand=np.zeros(n, np.uint8) if strand else None,
                                 offsets=np.zeros(n_reads + 1, np.uint64))


@pytest.mark.parametrize("total", [0, 3])
def test_seed_chains(total):
    pairs, q, db = np.ones((3, 2), np.uint32), minimizers(4), minimizers(5, 3, strand=False)
    answers = {"kmu_seed_chains": {-1: total}}
    known = dict(pairs=pairs, qpos=q.pos, qread=q.read, qstrand=q.strand, dbpos=db.pos, dbread=db.read)
    ret, calls = drive(lambda c: c.seed_chains(pairs, q, None, 15, 100, 20, min_seeds=2, min_score=30, max_pos=999, upper=True), known, answers)
    lead = ("kmu_seed_chains", "ctx", "pairs", 3, "qpos", "qread", "qstrand", 4, 2, "qpos", "qread", "qstrand", 4, 2,
            ("ChainParams", 15, 100, 20, 2, 30, 999, A.CHAIN_UPPER), A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    shapes(ret, (A.CHAIN_DTYPE, (total,)))
    ret, calls = drive(lambda c: c.seed_chains(pairs, q, db, 15, 100, 20), known, answers)
    lead = ("kmu_seed_chains", "ctx", "pairs", 3, "qpos", "qread", "qstrand", 4, 2, "dbpos", "dbread", None, 5, 3,
            ("ChainParams", 15, 100, 20, 1, 0, 0, 0), A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    e, eq = np.ones((0, 2), np.uint32), minimizers(0)
    ret, calls = drive(lambda c: c.seed_chains(e, eq, None, 15, 100, 20), {}, answers)
    lead = ("kmu_seed_chains", "ctx", "#0", 0, "#0", "#0", None, 0, 2, "#0", "#0", None, 0, 2, ("ChainParams", 15, 100, 20, 1, 0, 0, 0), A.MEM_HOST)
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))


# ---- the chain calls: two batches, or the self-join on one ----
def batch(n_bases=10, off=(0, 4, 10)):
    return u8(n_bases), list(off)


@pytest.mark.parametrize("form", range(3))
def test_chain_align(form):
    chains, (bq, oq), (bdb, odb) = recs(3, CHAIN), batch(), batch(7, (0, 3, 5, 7))
    oq, odb = OFFSET_FORMS[form](oq), OFFSET_FORMS[form](odb)
    known = dict(chains=chains, bq=bq, bdb=bdb)
    ret, calls = drive(lambda c: c.chain_align(chains, bq, oq, band=32), known)
    same_calls(calls, [("kmu_chain_align", "ctx", "chains", 3, "bq", "#0", 2, "bq", "#0", 2, ("AlignParams", 32, 0), A.MEM_HOST, "ret0")])
    shapes(ret, (ALN, (3,)))
    ret, calls = drive(lambda c: c.chain_align(chains, bq, oq, bdb, odb), known)
    same_calls(calls, [("kmu_chain_align", "ctx", "chains", 3, "bq", "#0", 2, "bdb", "#1", 3, ("AlignParams", 64, 0), A.MEM_HOST, "ret0")])
    ret, calls = drive(lambda c: c.chain_align(chains, bq, oq, bdb, oq), known)  # (one offsets object for both: converted once)
    same_calls(calls, [("kmu_chain_align", "ctx", "chains", 3, "bq", "#0", 2, "bdb", "#0", 2, ("AlignParams", 64, 0), A.MEM_HOST, "ret0")])


def test_chain_align_empty_and_checks():
    e, (be, oe), (bdb, odb) = recs(0, CHAIN), batch(0, (0, 0, 0)), batch(7, (0, 3, 5, 7))
    ret, calls = drive(lambda c: c.chain_align(e, be, oe), dict(chains=e, bq=be))
    same_calls(calls, [("kmu_chain_align", "ctx", "#0", 0, "#0", "#1", 2, "#0", "#1", 2, ("AlignParams", 64, 0), A.MEM_HOST, "ret0")])
    shapes(ret, (ALN, (0,)))
    ret, calls = drive(lambda c: c.chain_align(e, be, oe, bdb, odb), dict(chains=e, bq=be, bdb=bdb))
    same_calls(calls, [("kmu_chain_align", "ctx", "#0", 0, "#0", "#1", 2, "bdb", "#2", 3, ("AlignParams", 64, 0), A.MEM_HOST, "ret0")])
    for name in ("chain_align", "chain_cigar"):
        raises("bases_db without offsets_db", lambda c: getattr(c, name)(e, be, oe, bdb))
    raises("bases_db without offsets_db", lambda c: c.chain_pileup(e, recs(0, ALN), np.zeros(0, np.uint32), np.zeros(1, np.uint64), be, oe, bdb))
    raises("bases_db without offsets_db",
           lambda c: c.chain_pile_ins(e, recs(0, ALN), np.zeros(0, np.uint32), np.zeros(1, np.uint64), be, oe, be, 0, bdb))


@pytest.mark.parametrize("total", [0, 3])
@pytest.mark.parametrize("form", range(3))
def test_chain_cigar_two_calls(total, form):
    chains, (bq, oq), (bdb, odb) = recs(3, CHAIN), batch(), batch(7, (0, 3, 5, 7))
    oq, odb = OFFSET_FORMS[form](oq), OFFSET_FORMS[form](odb)
    known, answers = dict(chains=chains, bq=bq, bdb=bdb), {"kmu_chain_cigar": {-1: total}}
    ret, calls = drive(lambda c: c.chain_cigar(chains, bq, oq, band=32, max_trace_bytes=4096), known, answers)
    lead = ("kmu_chain_cigar", "ctx", "chains", 3, "bq", "#0", 2, "bq", "#0", 2, ("CigarParams", 32, 0, 4096), A.MEM_HOST, "ret0", "ret2")
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret1", 3, REF)] if total else []))
    shapes(ret, (ALN, (3,)), (np.uint32, (total,)), (np.uint64, (4,)))
    ret, calls = drive(lambda c: c.chain_cigar(chains, bq, oq, bdb, odb), known, answers)
    lead = ("kmu_chain_cigar", "ctx", "chains", 3, "bq", "#0", 2, "bdb", "#1", 3, ("CigarParams", 64, 0, 0), A.MEM_HOST, "ret0", "ret2")
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret1", 3, REF)] if total else []))
    e, (be, oe) = recs(0, CHAIN), batch(0, (0, 0, 0))
    ret, calls = drive(lambda c: c.chain_cigar(e, be, oe), {}, answers)
    lead = ("kmu_chain_cigar", "ctx", "#0", 0, "#0", "#1", 2, "#0", "#1", 2, ("CigarParams", 64, 0, 0), A.MEM_HOST, "ret0", "ret2")
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret1", 3, REF)] if total else []))
    shapes(ret, (ALN, (0,)), (np.uint32, (total,)), (np.uint64, (1,)))


def test_chain_cigar_sized_by_aln():
    chains, (bq, oq) = recs(3, CHAIN), batch()
    aln = recs(3, ALN)
    aln["edit"], aln["flags"] = [1, 2, 9], [A.ALN_DONE, A.ALN_DONE | A.ALN_EXACT, 0]
    known = dict(chains=chains, bq=bq, aln=aln)
    ret, calls = drive(lambda c: c.chain_cigar(chains, bq, oq, aln=aln), known, {"kmu_chain_cigar": {-1: 5}})
    lead = ("kmu_chain_cigar", "ctx", "chains", 3, "bq", "#0", 2, "bq", "#0", 2, ("CigarParams", 64, 0, 0), A.MEM_HOST, "ret0", "ret2")
    same_calls(calls, [lead + ("ret1", 8, REF)])  # 2 edit + 1 runs for the two chains that were aligned
    shapes(ret, (ALN, (3,)), (np.uint32, (5,)), (np.uint64, (4,)))
    aln["flags"] = 0
    ret, calls = drive(lambda c: c.chain_cigar(chains, bq, oq, aln=aln), known)
    same_calls(calls, [lead + ("ret1", 0, REF)])  # (the one call is made even for no run at all)
    shapes(ret, (ALN, (3,)), (np.uint32, (0,)), (np.uint64, (4,)))
    raises("aln holds 2 records for 3 chains", lambda c: c.chain_cigar(chains, bq, oq, aln=aln[:2]))


def pile_inputs(n=3, n_ops=5):
    return recs(n, CHAIN), recs(n, ALN), np.ones(n_ops, np.uint32), np.zeros(n + 1, np.uint64)


BOTH = A.PILE_Q | A.PILE_DB


@pytest.mark.parametrize("form", range(3))
@pytest.mark.parametrize("sides", [A.PILE_Q, A.PILE_DB, BOTH])
def test_chain_pileup(sides, form):
    chains, aln, ops, opo = pile_inputs()
    (bq, oq), (bdb, odb) = batch(), batch(7, (0, 3, 5, 7))
    oq, odb = OFFSET_FORMS[form](oq), OFFSET_FORMS[form](odb)
    known = dict(chains=chains, aln=aln, ops=ops, opo=opo, bq=bq, bdb=bdb)
    q, db = bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)
    # the self-join: one table under both names
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, bq, oq, sides=sides), known)
    lead = ("kmu_chain_pileup", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bq", "#0", 2, ("PileupParams", sides), A.MEM_HOST)
    same_calls(calls, [lead + ("ret0" if q else None, ("ret0" if q else "ret1") if db else None)])
    shapes(ret, (np.uint32, (10, A.PILE_COLS)) if q else None, (np.uint32, (10, A.PILE_COLS)) if db else None)
    assert sides != BOTH or ret[0] is ret[1]
    # two batches: a table each
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, bq, oq, bdb, odb, sides=sides), known)
    lead = ("kmu_chain_pileup", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bdb", "#1", 3, ("PileupParams", sides), A.MEM_HOST)
    same_calls(calls, [lead + ("ret0" if q else None, "ret1" if db else None)])
    shapes(ret, (np.uint32, (10, A.PILE_COLS)) if q else None, (np.uint32, (7, A.PILE_COLS)) if db else None)
    # into: one table for the self-join, a pair otherwise; the tables come back as they are
    one, tq, tdb = np.zeros((10, A.PILE_COLS), np.uint32), np.zeros((10, A.PILE_COLS), np.uint32), np.zeros((7, A.PILE_COLS), np.uint32)
    known.update(one=one, tq=tq, tdb=tdb)
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, bq, oq, sides=sides, into=one), known)
    lead = ("kmu_chain_pileup", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bq", "#0", 2, ("PileupParams", sides), A.MEM_HOST)
    same_calls(calls, [lead + ("one" if q else None, "one" if db else None)])
    assert ret[0] is one and ret[1] is one
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, bq, oq, bdb, odb, sides=sides, into=(tq, tdb)), known)
    lead = ("kmu_chain_pileup", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bdb", "#1", 3, ("PileupParams", sides), A.MEM_HOST)
    same_calls(calls, [lead + ("tq" if q else None, "tdb" if db else None)])
    assert ret[0] is tq and ret[1] is tdb
    lacking = (None, tdb) if q else (tq, None)
    raises("into lacks the table of a side that is asked for",
           lambda c: c.chain_pileup(chains, aln, ops, opo, bq, oq, bdb, odb, sides=sides, into=lacking))


def test_chain_pileup_empty_and_checks():
    chains, aln, ops, opo = pile_inputs(0, 0)
    (be, oe), (bdb, odb) = batch(0, (0, 0, 0)), batch(0, (0, 0))
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, be, oe), dict(opo=opo))
    same_calls(calls, [("kmu_chain_pileup", "ctx", "#0", 0, "#0", "opo", "#0", 0, "#0", "#1", 2, "#0", "#1", 2, ("PileupParams", BOTH), A.MEM_HOST,
                        "#0", "#0")])
    shapes(ret, (np.uint32, (0, A.PILE_COLS)), (np.uint32, (0, A.PILE_COLS)))
    # two distinct empty batches: both tables get the one placeholder, which the library refuses ("one table for both sides needs
    # the two batches to be the same arrays") -- pinned as it is; chain_pile_ins has a second placeholder for this
    ret, calls = drive(lambda c: c.chain_pileup(chains, aln, ops, opo, be, oe, bdb, odb), dict(opo=opo))
    same_calls(calls, [("kmu_chain_pileup", "ctx", "#0", 0, "#0", "opo", "#0", 0, "#0", "#1", 2, "#0", "#2", 1, ("PileupParams", BOTH), A.MEM_HOST,
                        "#0", "#0")])
    assert ret[0] is not ret[1]
    chains, aln, ops, opo = pile_inputs()
    bq, oq = batch()
    for bad in ((chains, aln[:2], ops, opo), (chains, aln, ops, opo[:3])):
        raises("3 chains need 3 alignment records and 4 run offsets", lambda c: c.chain_pileup(*bad, bq, oq))
        raises("3 chains need 3 alignment records and 4 run offsets", lambda c: c.chain_pile_ins(*bad, bq, oq, u8(10), 4))


@pytest.mark.parametrize("form", range(3))
@pytest.mark.parametrize("sides", [A.PILE_Q, A.PILE_DB, BOTH])
def test_chain_pile_ins(sides, form):
    chains, aln, ops, opo = pile_inputs()
    (bq, oq), (bdb, odb) = batch(), batch(7, (0, 3, 5, 7))
    oq, odb = OFFSET_FORMS[form](oq), OFFSET_FORMS[form](odb)
    lq, ldb = np.ones(10, np.uint8), np.ones(7, np.uint8)
    known = dict(chains=chains, aln=aln, ops=ops, opo=opo, bq=bq, bdb=bdb, lq=lq, ldb=ldb)
    q, db = bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)
    P = ("PileupParams", sides)
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, lq, 4, sides=sides), known)
    lead = ("kmu_chain_pile_ins", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bq", "#0", 2, P, A.MEM_HOST)
    t_db = "ret0" if q else "ret1"
    same_calls(calls, [lead + ("lq" if q else None, 4, "ret0" if q else None, "lq" if db else None, 4, t_db if db else None)])
    shapes(ret, (np.uint32, (4, A.INS_COLS)) if q else None, (np.uint32, (4, A.INS_COLS)) if db else None)
    assert sides != BOTH or ret[0] is ret[1]
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, lq, 4, bdb, odb, ldb, 6, sides=sides), known)
    lead = ("kmu_chain_pile_ins", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bdb", "#1", 3, P, A.MEM_HOST)
    same_calls(calls, [lead + ("lq" if q else None, 4, "ret0" if q else None, "ldb" if db else None, 6, "ret1" if db else None)])
    shapes(ret, (np.uint32, (4, A.INS_COLS)) if q else None, (np.uint32, (6, A.INS_COLS)) if db else None)
    one, tq, tdb = np.zeros((4, A.INS_COLS), np.uint32), np.zeros((4, A.INS_COLS), np.uint32), np.zeros((6, A.INS_COLS), np.uint32)
    known.update(one=one, tq=tq, tdb=tdb)
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, lq, 4, sides=sides, into=one), known)
    lead = ("kmu_chain_pile_ins", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bq", "#0", 2, P, A.MEM_HOST)
    same_calls(calls, [lead + ("lq" if q else None, 4, "one" if q else None, "lq" if db else None, 4, "one" if db else None)])
    assert ret[0] is one and ret[1] is one
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, lq, 4, bdb, odb, ldb, 6, sides=sides, into=[tq, tdb]), known)
    lead = ("kmu_chain_pile_ins", "ctx", "chains", 3, "aln", "opo", "ops", 5, "bq", "#0", 2, "bdb", "#1", 3, P, A.MEM_HOST)
    same_calls(calls, [lead + ("lq" if q else None, 4, "tq" if q else None, "ldb" if db else None, 6, "tdb" if db else None)])
    assert ret[0] is tq and ret[1] is tdb
    lacking = (None, tdb) if q else (tq, None)
    raises("into lacks the table of a side that is asked for",
           lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, lq, 4, bdb, odb, ldb, 6, sides=sides, into=lacking))
    no_plan = dict(ins_len_q=None, n_slots_q=None, ins_len_db=ldb, n_slots_db=6) if q else dict(ins_len_q=lq, n_slots_q=4)
    raises("a side that is asked for needs its ins_len and n_slots",
           lambda c: c.chain_pile_ins(chains, aln, ops, opo, bq, oq, bases_db=bdb, offsets_db=odb, sides=sides, **no_plan))


@pytest.mark.parametrize("sides", [A.PILE_Q, A.PILE_DB, BOTH])
def test_chain_pile_ins_empty(sides):
    """an empty batch: every input is the one placeholder, and two empty tables are still two addresses"""
    chains, aln, ops, opo = pile_inputs(0, 0)
    (be, oe), (bdb, odb) = batch(0, (0, 0, 0)), batch(0, (0, 0))
    le, q, db = np.zeros(0, np.uint8), bool(sides & A.PILE_Q), bool(sides & A.PILE_DB)
    P = ("PileupParams", sides)
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, be, oe, le, 0, sides=sides), dict(opo=opo))
    lead = ("kmu_chain_pile_ins", "ctx", "#0", 0, "#0", "opo", "#0", 0, "#0", "#1", 2, "#0", "#1", 2, P, A.MEM_HOST)
    # the self-join with both sides has one table; with the B side alone the table is not the (absent) A table
    same_calls(calls, [lead + ("#0" if q else None, 0, "#0" if q else None, "#0" if db else None, 0, ("#0" if q else "#2") if db else None)])
    shapes(ret, (np.uint32, (0, A.INS_COLS)) if q else None, (np.uint32, (0, A.INS_COLS)) if db else None)
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, be, oe, le, None, bdb, odb, le.copy(), None, sides=sides), dict(opo=opo))
    lead = ("kmu_chain_pile_ins", "ctx", "#0", 0, "#0", "opo", "#0", 0, "#0", "#1", 2, "#0", "#2", 1, P, A.MEM_HOST)
    same_calls(calls, [lead + ("#0" if q else None, 0, "#0" if q else None, "#0" if db else None, 0, "#3" if db else None)])
    one = np.zeros((0, A.INS_COLS), np.uint32)
    ret, calls = drive(lambda c: c.chain_pile_ins(chains, aln, ops, opo, be, oe, le, 0, sides=sides, into=one), dict(opo=opo))
    lead = ("kmu_chain_pile_ins", "ctx", "#0", 0, "#0", "opo", "#0", 0, "#0", "#1", 2, "#0", "#1", 2, P, A.MEM_HOST)
    same_calls(calls, [lead + ("#0" if q else None, 0, "#0" if q else None, "#0" if db else None, 0, "#0" if db else None)])


# ---- pile calls, plans, consensus, segments, ranges ----
def test_pile_call():
    pile, (bases, off) = np.zeros((10, A.PILE_COLS), np.uint32), batch()
    known = dict(pile=pile, bases=bases)
    ret, calls = drive(lambda c: c.pile_call(pile, bases, off, min_depth=5), known)
    same_calls(calls, [("kmu_pile_call", "ctx", "pile", "bases", "#0", 2, ("PileCallParams", 5, 0), A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint8, (10,)), (A.READ_PILE_DTYPE, (2,)))
    ret, calls = drive(lambda c: c.pile_call(pile, bases, np.array(off, np.uint64), want=("reads",)), known)
    same_calls(calls, [("kmu_pile_call", "ctx", "pile", "bases", "#0", 2, ("PileCallParams", 3, 0), A.MEM_HOST, None, "ret1")])
    shapes(ret, None, (A.READ_PILE_DTYPE, (2,)))
    ret, calls = drive(lambda c: c.pile_call(pile, bases, off, want=("call",)), known)
    same_calls(calls, [("kmu_pile_call", "ctx", "pile", "bases", "#0", 2, ("PileCallParams", 3, 0), A.MEM_HOST, "ret0", None)])
    e = np.zeros((0, A.PILE_COLS), np.uint32)
    ret, calls = drive(lambda c: c.pile_call(e, u8(0), [0]), {})
    same_calls(calls, [("kmu_pile_call", "ctx", "#0", "#0", "#1", 0, ("PileCallParams", 3, 0), A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint8, (0,)), (A.READ_PILE_DTYPE, (0,)))
    raises("want holds ['calls']: the outputs are ('call', 'reads'), at least one", lambda c: c.pile_call(pile, bases, off, want=["calls"]))
    raises("want holds []: the outputs are ('call', 'reads'), at least one", lambda c: c.pile_call(pile, bases, off, want=()))
    raises("the batch has 10 bases: the table and the bases must have as many rows", lambda c: c.pile_call(pile[:9], bases, off))


def test_pile_ins_plan():
    pile, call = np.zeros((10, A.PILE_COLS), np.uint32), np.zeros(10, np.uint8)
    ret, calls = drive(lambda c: c.pile_ins_plan(pile, call, max_ins=7), dict(pile=pile, call=call), {"kmu_pile_ins_plan": {-1: 12}})
    same_calls(calls, [("kmu_pile_ins_plan", "ctx", "pile", "call", 10, ("InsPlanParams", 7, 0), A.MEM_HOST, "ret0", REF)])
    shapes(ret[:1], (np.uint8, (10,)))
    assert ret[1] == 12 and type(ret[1]) is int
    ret, calls = drive(lambda c: c.pile_ins_plan(pile[:0], call[:0]), {})
    same_calls(calls, [("kmu_pile_ins_plan", "ctx", "#0", "#0", 0, ("InsPlanParams", 16, 0), A.MEM_HOST, "ret0", REF)])
    shapes(ret[:1], (np.uint8, (0,)))
    raises("the table has 10 rows: call must have as many bytes", lambda c: c.pile_ins_plan(pile, call[:9]))


def consensus_inputs(n_bases=10, n_slots=4, off=(0, 4, 10)):
    x = dict(pile=np.zeros((n_bases, A.PILE_COLS), np.uint32), call=np.zeros(n_bases, np.uint8), ins_len=np.zeros(n_bases, np.uint8),
             ins=np.zeros((n_slots, A.INS_COLS), np.uint32), bases=u8(n_bases))
    return x, (x["pile"], x["call"], x["ins_len"], n_slots, x["ins"], x["bases"], list(off))


def test_pile_consensus():
    known, args = consensus_inputs()
    ret, calls = drive(lambda c: c.pile_consensus(*args), known, {"kmu_pile_consensus": {-1: 12}})
    same_calls(calls, [("kmu_pile_consensus", "ctx", "pile", "call", "ins_len", 4, "ins", "bases", "#0", 2, ("ConsensusParams", 0), A.MEM_HOST,
                        "ret1", "ret0", 14, REF)])
    shapes(ret, (np.uint8, (12,)), (np.uint64, (3,)))
    known, args = consensus_inputs(0, 0, (0, 0, 0))
    ret, calls = drive(lambda c: c.pile_consensus(*args), known)
    same_calls(calls, [("kmu_pile_consensus", "ctx", "#0", "#0", "#0", 0, "#0", "#0", "#1", 2, ("ConsensusParams", 0), A.MEM_HOST,
                        "ret1", "ret0", 0, REF)])
    shapes(ret, (np.uint8, (0,)), (np.uint64, (3,)))


def test_pile_consensus_pos():
    known, args = consensus_inputs()
    rows = np.array([0, 4, 10], np.uint64)
    ret, calls = drive(lambda c: c.pile_consensus_pos(*args, rows), dict(known, rows=rows))
    same_calls(calls, [("kmu_pile_consensus_pos", "ctx", "pile", "call", "ins_len", 4, "ins", "bases", "#0", 2, ("ConsensusParams", 0),
                        A.MEM_HOST, "#1", 3, "ret0")])  # (rows are converted: a copy)
    shapes(ret, (np.uint64, (3,)))
    known, args = consensus_inputs(0, 0, (0, 0, 0))
    ret, calls = drive(lambda c: c.pile_consensus_pos(*args, np.zeros(0, np.int64)), known)
    same_calls(calls, [("kmu_pile_consensus_pos", "ctx", "#0", "#0", "#0", 0, "#0", "#0", "#1", 2, ("ConsensusParams", 0), A.MEM_HOST,
                        "#0", 0, "ret0")])
    shapes(ret, (np.uint64, (0,)))


@pytest.mark.parametrize("name", ["pile_consensus", "pile_consensus_pos"])
def test_consensus_checks(name):
    known, args = consensus_inputs()
    more = (np.zeros(2, np.uint64),) if name == "pile_consensus_pos" else ()
    for at in (0, 1, 2, 5):
        bad = list(args)
        bad[at] = bad[at][:9]
        raises("the batch has 10 bases: the table, call, ins_len and the bases must have as many rows", lambda c: getattr(c, name)(*bad, *more))
    bad = list(args)
    bad[3] = 5
    raises("ins has 4 slots, not n_slots = 5", lambda c: getattr(c, name)(*bad, *more))


def test_pile_segments():
    pile, off = np.zeros((10, A.PILE_COLS), np.uint32), [0, 4, 10]
    ret, calls = drive(lambda c: c.pile_segments(pile, off, min_len=3), dict(pile=pile), {"kmu_pile_segments": {9: 2}})
    same_calls(calls, [("kmu_pile_segments", "ctx", "pile", "#0", 2, ("PileSegParams", 3, 3, 3, 0), A.MEM_HOST, "ret1", "ret0", 3, REF, "ret2")])
    shapes(ret, (A.PILE_SEG_DTYPE, (2,)), (np.uint64, (3,)), (A.READ_TRIM_DTYPE, (2,)))
    ret, calls = drive(lambda c: c.pile_segments(pile, off, min_depth=4, min_span=0, longest=True), dict(pile=pile))
    same_calls(calls, [("kmu_pile_segments", "ctx", "pile", "#0", 2, ("PileSegParams", 4, 0, 1, A.SEG_LONGEST), A.MEM_HOST, "ret1", "ret0", 2, REF,
                        "ret2")])
    ret, calls = drive(lambda c: c.pile_segments(pile[:0], [0]), {})
    same_calls(calls, [("kmu_pile_segments", "ctx", "#0", "#1", 0, ("PileSegParams", 3, 3, 1, 0), A.MEM_HOST, "ret1", "ret0", 0, REF, "ret2")])
    shapes(ret, (A.PILE_SEG_DTYPE, (0,)), (np.uint64, (1,)), (A.READ_TRIM_DTYPE, (0,)))
    raises("the batch has 10 bases: the table must have as many rows", lambda c: c.pile_segments(pile[:9], off))


@pytest.mark.parametrize("total", [0, 3])
def test_extract_ranges(total):
    bases, begin, end = u8(10), np.array([0, 2], np.int64), np.array([1, 4], np.int64)
    answers = {"kmu_extract_ranges": {-1: total}}
    ret, calls = drive(lambda c: c.extract_ranges(bases, begin, end), dict(bases=bases), answers)
    lead = ("kmu_extract_ranges", "ctx", "bases", 10, "#0", "#1", 2, A.MEM_HOST, "ret1")
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    shapes(ret, (np.uint8, (total,)), (np.uint64, (3,)))
    ret, calls = drive(lambda c: c.extract_ranges(u8(0), begin[:0], end[:0]), {}, answers)
    lead = ("kmu_extract_ranges", "ctx", "#0", 0, "#0", "#0", 0, A.MEM_HOST, "ret1")
    same_calls(calls, [lead + (None, 0, REF)] + ([lead + ("ret0", 3, REF)] if total else []))
    raises("2 begins need as many ends", lambda c: c.extract_ranges(bases, begin, end[:1]))


# ---- string graph ----
def test_sg_classify():
    chains, aln, off = recs(3, CHAIN), recs(3, ALN), [0, 4, 10]
    ret, calls = drive(lambda c: c.sg_classify(chains, aln, off, min_overlap=100, fuzz=7), dict(chains=chains, aln=aln))
    same_calls(calls, [("kmu_sg_classify", "ctx", "chains", "aln", 3, "#0", 2, ("SgParams", 100, 1000, 250, 0, 7, 0), A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint8, (3,)), (A.SG_READ_DTYPE, (2,)))
    ret, calls = drive(lambda c: c.sg_classify(chains[:0], aln[:0], [0]), {})
    same_calls(calls, [("kmu_sg_classify", "ctx", "#0", None, 0, "#1", 0, ("SgParams", 500, 1000, 250, 0, 10, 0), A.MEM_HOST, "ret0", "ret1")])
    shapes(ret, (np.uint8, (0,)), (A.SG_READ_DTYPE, (0,)))
    raises("3 chains need as many alignment records", lambda c: c.sg_classify(chains, aln[:2], off))


@pytest.mark.parametrize("total", [0, 3])
def test_sg_graph(total):
    chains, off = recs(3, CHAIN), [0, 4, 10]
    ret, calls = drive(lambda c: c.sg_graph(chains, None, off), dict(chains=chains), {"kmu_sg_graph": {-1: total}})
    lead = ("kmu_sg_graph", "ctx", "chains", None, 3, "#0", 2, ("SgParams", 500, 1000, 250, 0, 10, 0), A.MEM_HOST)
    same_calls(calls, [lead + (None, None, None, 0, None, REF), lead + ("ret2", "ret3", "ret0", total, "ret1", REF)])  # (always twice)
    shapes(ret, (A.SG_ARC_DTYPE, (total,)), (np.uint64, (5,)), (np.uint8, (3,)), (A.SG_READ_DTYPE, (2,)))


def test_sg_unitigs_and_clean():
    arcs, reads, off = recs(4, A.SG_ARC_DTYPE), recs(2, A.SG_READ_DTYPE), [0, 4, 10]
    ret, calls = drive(lambda c: c.sg_unitigs(arcs, reads, off), dict(arcs=arcs, reads=reads), {"kmu_sg_unitigs": {10: 2, 11: 1}})
    same_calls(calls, [("kmu_sg_unitigs", "ctx", "arcs", 4, "reads", "#0", 2, A.MEM_HOST, "ret0", "ret1", "ret2", REF, REF)])
    shapes(ret, (A.SG_UNITIG_DTYPE, (1,)), (A.SG_STEP_DTYPE, (2,)), (A.SG_PLACE_DTYPE, (2,)))
    ret, calls = drive(lambda c: c.sg_unitigs(arcs[:0], None, [0]), {})
    same_calls(calls, [("kmu_sg_unitigs", "ctx", "#0", 0, None, "#1", 0, A.MEM_HOST, "ret0", "ret1", "ret2", REF, REF)])
    raises("2 reads need as many summaries", lambda c: c.sg_unitigs(arcs, reads[:1], off))
    ret, calls = drive(lambda c: c.sg_clean(arcs, reads, 2, max_tip_reads=3), dict(arcs=arcs, reads=reads))
    same_calls(calls, [("kmu_sg_clean", "ctx", "arcs", 4, "reads", 2, ("SgCleanParams", 3, 8, 0, 0), A.MEM_HOST, "ret0", "ret1", REF)])
    shapes(ret[:2], (A.SG_ARC_DTYPE, (4,)), (A.SG_READ_DTYPE, (2,)))
    assert ret[2] == {name: 0 for name in A.SG_CLEAN_STATS}
    ret, calls = drive(lambda c: c.sg_clean(arcs[:0], None, 0), {})
    same_calls(calls, [("kmu_sg_clean", "ctx", "#0", 0, None, 0, ("SgCleanParams", 4, 8, 0, 0), A.MEM_HOST, "ret0", "ret1", REF)])
    shapes(ret[:2], (A.SG_ARC_DTYPE, (0,)), (A.SG_READ_DTYPE, (0,)))
    raises("2 reads need as many summaries", lambda c: c.sg_clean(arcs, reads[:1], 2))


def test_sg_unitig_chains():
    unitigs, path, place = recs(1, A.SG_UNITIG_DTYPE), recs(2, A.SG_STEP_DTYPE), recs(2, A.SG_PLACE_DTYPE)
    chains, classes, off = recs(3, CHAIN), np.zeros(3, np.uint8), [0, 4, 10]
    known = dict(unitigs=unitigs, path=path, place=place, chains=chains, classes=classes)
    ret, calls = drive(lambda c: c.sg_unitig_chains(unitigs, path, place, chains, classes, off), known, {"kmu_sg_unitig_chains": {-1: 1}})
    same_calls(calls, [("kmu_sg_unitig_chains", "ctx", "unitigs", 1, "path", 2, "place", "chains", "classes", 3, "#0", 2, ("UmParams", 0, 0),
                        A.MEM_HOST, "ret0", REF, REF)])
    shapes(ret[:1], (A.CHAIN_DTYPE, (1,)))
    assert ret[1] == {name: 0 for name in A.UM_STATS}
    ret, calls = drive(lambda c: c.sg_unitig_chains(unitigs[:0], path[:0], place[:0], None, None, [0]), {})
    same_calls(calls, [("kmu_sg_unitig_chains", "ctx", "#0", 0, "#0", 0, "#0", None, None, 0, "#1", 0, ("UmParams", 0, 0), A.MEM_HOST, "ret0", REF,
                        REF)])
    raises("chains and classes come together", lambda c: c.sg_unitig_chains(unitigs, path, place, chains, None, off))
    raises("3 chains need as many classes", lambda c: c.sg_unitig_chains(unitigs, path, place, chains, classes[:2], off))
    raises("2 reads need as many places", lambda c: c.sg_unitig_chains(unitigs, path, place[:1], chains, classes, off))


@pytest.mark.parametrize("total", [0, 3])
def test_sg_unitig_seqs(total):
    unitigs, path, (bases, off) = recs(1, A.SG_UNITIG_DTYPE), recs(2, A.SG_STEP_DTYPE), batch()
    answers = {"kmu_sg_unitig_seqs": {-1: total}}
    ret, calls = drive(lambda c: c.sg_unitig_seqs(unitigs, path, bases, off), dict(unitigs=unitigs, path=path, bases=bases), answers)
    lead = ("kmu_sg_unitig_seqs", "ctx", "unitigs", 1, "path", 2, "bases", "#0", 2, A.MEM_HOST)
    same_calls(calls, [lead + (None, None, 0, REF), lead + ("ret1", "ret0", total, REF)])  # (always twice: the second writes the offsets)
    shapes(ret, (np.uint8, (total,)), (np.uint64, (2,)))
    ret, calls = drive(lambda c: c.sg_unitig_seqs(unitigs[:0], path[:0], u8(0), [0]), {}, answers)
    lead = ("kmu_sg_unitig_seqs", "ctx", "#0", 0, "#0", 0, "#0", "#1", 0, A.MEM_HOST)
    same_calls(calls, [lead + (None, None, 0, REF), lead + ("ret1", "ret0", total, REF)])


# ---- components ----
def test_components():
    edges = np.ones((3, 2), np.uint32)
    ret, calls = drive(lambda c: c.components(edges, 5, weight_at=1, min_weight=2), dict(edges=edges), {"kmu_components": {-1: 2}})
    same_calls(calls, [("kmu_components", "ctx", 5, "edges", 3, 2, 1, 2, A.MEM_HOST, "ret0", "ret1", "ret2", "ret3", REF)])
    shapes(ret[:4], (np.uint32, (5,)), (np.uint32, (5,)), (np.uint32, (2,)), (np.uint32, (5,)))
    assert ret[4] == 2
    ret, calls = drive(lambda c: c.components(edges[:0], 5, want=("size",), count=False), {})
    same_calls(calls, [("kmu_components", "ctx", 5, "#0", 0, 2, 0, 0, A.MEM_HOST, "ret0", None, "ret2", None, None)])
    shapes(ret[:4], (np.uint32, (5,)), None, (np.uint32, (5,)), None)
    idx = np.ones((3, 2), np.uint32)
    ret, calls = drive(lambda c: c.components_knn(idx, None, min_eq=3), dict(idx=idx), {"kmu_components_knn": {-1: 1}})
    same_calls(calls, [("kmu_components_knn", "ctx", 3, "idx", None, 2, 3, A.MEM_HOST, "ret0", "ret1", "ret2", "ret3", REF)])
    ret, calls = drive(lambda c: c.components_knn(idx[:0], None), {})
    same_calls(calls, [("kmu_components_knn", "ctx", 0, "#0", None, 2, 0, A.MEM_HOST, "ret0", "ret1", "ret2", "ret3", REF)])


# ---- k-mers, counter, prefilter ----
@pytest.mark.parametrize("total", [0, 3])
@pytest.mark.parametrize("want", [("pos", "read", "strand"), ("pos",), ()])
def test_read_minimizers(total, want):
    """the count call writes the offsets; the second call is made for a total of 0 only where a strand is asked for"""
    hp = ("HashParams", A.KMER32BIT, 5, A.FHASH_CANON_RAW, A.INPUT_ASCII, A.MEM_HOST, 0)
    outs = tuple(("ret%d" % (i + 1)) if name in want else None for i, name in enumerate(lib.MINIMIZERS_WANT))
    kinds = ((np.uint64, (total,)),) + tuple((t, (total,)) if name in want else None
                                             for name, t in zip(lib.MINIMIZERS_WANT, (np.uint32, np.uint32, np.uint8)))
    for bases, off, p_bases in ((u8(10), np.array([0, 4, 10], np.uint64), "bases"), (u8(0), np.zeros(3, np.uint64), "#0")):
        ret, calls = drive(lambda c: c.read_minimizers(bases, off, A.KMER32BIT, 5, A.FHASH_CANON_RAW, 4, want=want), dict(bases=bases, off=off),
                           {"kmu_read_minimizers": {-1: total}})
        lead = ("kmu_read_minimizers", "ctx", hp, p_bases, "off", 2, 4)
        second = [lead + ("ret0",) + outs + (total, None, REF)] if total or "strand" in want else []
        same_calls(calls, [lead + (None, None, None, None, 0, "ret4", REF)] + second)
        shapes(ret, *kinds, (np.uint64, (3,)))
    raises("want holds ['hash']: the optional outputs are ('pos', 'read', 'strand')",
           lambda c: c.read_minimizers(bases, off, A.KMER32BIT, 5, A.FHASH_CANON_RAW, 4, want=("pos", "hash")))


def test_count_non_acgt():
    bases, off = u8(10), np.array([0, 4, 10], np.uint64)
    ret, calls = drive(lambda c: c.count_non_acgt(bases, off), dict(bases=bases, off=off))
    same_calls(calls, [("kmu_count_non_acgt", "ctx", "bases", "off", 2, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint64, (2,)))
    ret, calls = drive(lambda c: c.count_non_acgt(bases, off[:1]), dict(bases=bases, off=off))
    same_calls(calls, [("kmu_count_non_acgt", "ctx", "bases", "off", 0, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint64, (0,)))


@pytest.mark.parametrize("total", [0, 3])
def test_kmer_two_calls(total):
    bases, off = u8(10), np.array([0, 4, 10], np.uint64)
    known = dict(bases=bases, off=off)
    hp = ("HashParams", A.KMER32BIT, 5, A.FHASH_CANON_RAW, A.INPUT_ASCII, A.MEM_HOST, 0)
    ret, calls = drive(lambda c: c.kmer_hashes_compact(bases, off, A.KMER32BIT, 5, A.FHASH_CANON_RAW), known, {"kmu_kmer_hashes_compact": {-1: total}})
    lead = ("kmu_kmer_hashes_compact", "ctx", hp, "bases", "off", None, 2)
    same_calls(calls, [lead + (None, 0, REF), lead + ("ret0", total, REF)])
    shapes(ret, (np.uint64, (total,)))
    ret, calls = drive(lambda c: c.kmer_distribution(bases, off, A.KMER32BIT, 5, A.FHASH_CANON_RAW), known, {"kmu_kmer_distribution": {-1: total}})
    lead = ("kmu_kmer_distribution", "ctx", hp, "bases", "off", None, 2)
    same_calls(calls, [lead + (None, None, 0, None, REF), lead + ("ret0", "ret1", total, "ret2", REF)])
    shapes(ret, (np.uint64, (total,)), (np.uint32, (total,)), (np.uint64, (3,)))


def counter(ctx):
    return handle(lib.Counter, ctx, p=A.CountParams(A.KMER32BIT, 5, 8, 0, 1 << 10))


def test_counter_query():
    canon = np.arange(3, dtype=np.uint64)
    ret, calls = drive(lambda c: counter(c).query(canon), dict(canon=canon))
    same_calls(calls, [("kmu_count_query", "h", "canon", 3, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint32, (3,)))
    ret, calls = drive(lambda c: counter(c).query(canon.astype(np.int64)), {})  # (converted: a copy)
    same_calls(calls, [("kmu_count_query", "h", "#0", 3, A.MEM_HOST, "ret0")])
    ret, calls = drive(lambda c: counter(c).query(canon[:0]), {})
    assert calls[0][:1] + calls[0][3:] == ("kmu_count_query", 0, A.MEM_HOST, "ret0") and calls[0][2] is not None
    shapes(ret, (np.uint32, (0,)))


@pytest.mark.parametrize("total", [0, 3])
def test_counter_two_calls(total):
    ret, calls = drive(lambda c: counter(c).dump(min_count=3), {}, {"kmu_count_dump": {-1: total}})
    same_calls(calls, [("kmu_count_dump", "h", 3, None, None, 0, REF), ("kmu_count_dump", "h", 3, "ret0", "ret1", total, REF)])
    shapes(ret, (np.uint64, (total,)), (np.uint32, (total,)))
    bases, off = u8(10), np.array([0, 4, 10], np.uint64)
    ret, calls = drive(lambda c: counter(c).once_positions(bases, off), dict(bases=bases, off=off), {"kmu_count_once_positions": {-1: total}})
    lead = ("kmu_count_once_positions", "h", "bases", "off", 2, A.MEM_HOST)
    same_calls(calls, [lead + (None, None, None, 0, REF), lead + ("ret0", "ret1", "ret2", total, REF)])
    shapes(ret, (np.uint64, (total,)), (np.uint32, (total,)), (np.uint32, (total,)))


def test_counter_close():
    ctx = context()
    cnt = counter(ctx)
    cnt.close()
    cnt.close()
    assert cnt.h is None and [c[0] for c in ctx.L.calls] == ["kmu_count_destroy"]
    cnt = counter(ctx)
    ctx.h = None
    cnt.close()  # after the context: silent
    assert cnt.h is None and len(ctx.L.calls) == 1


def kfilter(ctx):
    return handle(lib.KFilter, ctx, p=A.KFilterParams(A.KMER32BIT, 5, 4, 0, 64))


def test_kfilter():
    canon, bases, off = np.arange(3, dtype=np.uint64), u8(10), np.array([0, 4, 10], np.uint64)
    known = dict(canon=canon, bases=bases, off=off)
    ret, calls = drive(lambda c: kfilter(c).query(canon), known)
    same_calls(calls, [("kmu_kfilter_query", "h", "canon", 3, A.MEM_HOST, "ret0")])
    shapes(ret, (np.uint8, (3,)))
    ret, calls = drive(lambda c: kfilter(c).query(canon[:0]), {})
    shapes(ret, (np.uint8, (0,)))
    for total, got in ((0, 0), (3, 3), (3, 2)):
        ret, calls = drive(lambda c: select(c, bases, off, total, got), known)
        lead = ("kmu_kfilter_select_reads", "h", "bases", "off", 2, A.MEM_HOST)
        same_calls(calls, [lead + (None, 0, REF), lead + ("ret0", total, REF)])
        shapes(ret, (np.uint64, (got,)))
    ret, calls = drive(lambda c: kfilter(c).n_passing(bases, off), known, {"kmu_kfilter_select_reads": {-1: 5}})
    same_calls(calls, [("kmu_kfilter_select_reads", "h", "bases", "off", 2, A.MEM_HOST, None, 0, REF)])
    assert ret == (5,)
    ret, calls = drive(lambda c: kfilter(c).export(), {})
    same_calls(calls, [("kmu_kfilter_export", "h", "ret0", A.MEM_HOST)])
    shapes(ret, (np.uint64, (128,)))
    with kfilter(context()) as f:
        L = f.L
    assert f.h is None and [c[0] for c in L.calls] == ["kmu_kfilter_destroy"]


def select(ctx, bases, off, total, got):
    """KFilter.select_reads on a stand-in whose size query answers `total` and whose writing call answers `got`"""
    seq = [total, got]
    rec = ctx.L

    class Answering:
        def __getattr__(self, name):
            fn = getattr(rec, name)

            def call(*args):
                rc = fn(*args)
                args[-1]._obj.value = seq.pop(0)
                return rc
            return call
    f = kfilter(ctx)
    f.L = Answering()
    return f.select_reads(bases, off)

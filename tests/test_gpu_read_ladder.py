"""-m gpu: the long-read route on hostile batches, every stage against its reference.  tests/read_families.py has the batches
(tandem repeats, homopolymers, identical reads, a palindrome, dovetails, unrelated reads, empty and short reads, lower case, a chimera
joined on opposite strands) and the two ladders; tests/test_read_ladder_ref.py shows on the references alone that the batches
produce what they are there for -- chains without DONE, EXACT or PATH out of the chaining itself, no chains at all, a split at a
join.  Here the device walks the same route: each stage's output is compared byte for byte with that stage's reference applied to
the device's own output of the stage before, the one-call wrappers of kmerutils_amd.minimizer are compared with the ladder, on host
arrays and on resident tensors, and the route is run over two batches, a second time over its own output, and over all families in
one batch."""
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import read_families as RF  # noqa: E402
from read_families import CASES, DEFAULT, FAMILIES, K, W, batch, case_batch, check_ladder, device_ladder, flag_counts  # noqa: E402
from test_gpu_chain_pileup import same_table  # noqa: E402
from test_gpu_minimizers import expected, same as same_minimizers  # noqa: E402
from test_gpu_pile_segments import same  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ladders(ctx):
    """the device ladder of a case, computed once"""
    done = {}

    def get(name):
        if name not in done:
            bases, offsets, params = case_batch(name)
            done[name] = device_ladder(ctx, bases, offsets, params)
        return done[name]
    return get


def on_device(bases, offsets):
    import torch
    return torch.from_numpy(np.ascontiguousarray(bases)).cuda(), torch.from_numpy(np.asarray(offsets).astype(np.int64)).cuda()


def raw(x):
    """the bytes of a result, wherever it lives"""
    if isinstance(x, int):
        return x
    return (x.cpu().numpy() if hasattr(x, "cpu") else np.ascontiguousarray(x)).tobytes()


def chain_kw(p):
    return dict(max_occ=p.max_occ, max_gap=p.max_gap, min_seeds=p.min_seeds, min_score=p.min_score)


def wrappers(ctx, bases, offsets, p, longest=False):
    """the five one-call routes of kmerutils_amd.minimizer under the parameters of a ladder, as a dict of result tuples"""
    align = dict(chain_kw(p), band_chain=p.band_chain, band=p.band, max_trace_bytes=p.max_trace_bytes)
    return {
        "read_chains": (minimizer.read_chains(ctx, bases, offsets, p.k, p.w, band=p.band_chain, **chain_kw(p)),),
        "read_cigars": minimizer.read_cigars(ctx, bases, offsets, p.k, p.w, **align),
        "read_pileups": minimizer.read_pileups(ctx, bases, offsets, p.k, p.w, min_depth=p.min_depth, **align),
        "correct_reads": minimizer.correct_reads(ctx, bases, offsets, p.k, p.w, min_depth=p.min_depth, max_ins=p.max_ins, **align),
        "correct_trim_reads": minimizer.correct_trim_reads(ctx, bases, offsets, p.k, p.w, min_depth=p.min_depth, max_ins=p.max_ins, min_span=p.min_span,
                                                           min_len=p.min_len, longest=longest, **align),
    }


def of_ladder(lad):
    """what the wrappers return, taken from a ladder over one batch"""
    return {
        "read_chains": (lad.chains,),
        "read_cigars": (lad.chains, lad.aln, lad.ops, lad.op_off),
        "read_pileups": (lad.chains, lad.aln, lad.pile[0], lad.call[0], lad.reads[0]),
        "correct_reads": (lad.cons[0], lad.cons_off[0], lad.reads[0]),
        "correct_trim_reads": (lad.out[0], lad.out_off[0], lad.segs[0], lad.reads[0], lad.trims[0]),
    }


def equal_results(got, want, what):
    for name in want:
        assert len(got[name]) == len(want[name]), (what, name)
        for k, (g, w) in enumerate(zip(got[name], want[name])):
            assert raw(g) == raw(w), "%s: %s, result %d differs from the ladder's" % (what, name, k)


# ---- every stage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_of_every_family(ctx, oracle, ladders, name):
    bases, offsets, params = case_batch(name)
    lad = ladders(name)
    # the minimizers against the oracle's k-mer hashes, with the helpers of their own test; then every stage in turn
    same_minimizers(lad.mini[0][:5], expected(oracle, bases if bases.size else np.zeros(1, np.uint8), offsets, RF.KMER_TYPE, K, RF.FHASH, W), name)
    check_ladder(lad, oracle, params, name)
    same_table(lad.pile[0], RF.reference_stage(lad, "chain_pileup", params)["pile"][0], name)
    for what, want in RF.reference_stage(lad, "pile_segments", params).items():
        same(getattr(lad, what)[0], want[0], "%s %s" % (name, what))
    counts = flag_counts(lad.aln)
    print("%s: %d pairs, %s" % (name, len(lad.pairs), counts))
    # the conditions tests/test_read_ladder_ref.py asserts on the references, on the device's records
    if name == "tandem_flags":
        assert RF.has_every_flag_state(lad.aln), counts
        assert counts["no DONE"] >= 1 and counts["no EXACT"] > counts["no DONE"] and counts["no PATH"] > counts["no DONE"] and counts["all"] >= 1
    if name in ("tandem", "homopolymer"):
        assert counts["no EXACT"] >= 1 and counts["all"] >= 1
    if name == "tandem_occ8":
        assert 0 < len(lad.pairs) < len(ladders("tandem").pairs) and len(lad.chains) > 0
    if name == "unrelated":
        assert lad.pairs.shape == (0, 2) and len(lad.chains) == 0 and not lad.pile[0].any() and lad.cons[0].tobytes() == bases.tobytes()
        assert (lad.trims[0]["cls"] == A.TRIM_NONE).all() and lad.n_slots[0] == 0
    if name == "identical":
        assert (lad.aln["edit"] == 0).all() and lad.cons[0].tobytes() == bases.tobytes() and (lad.trims[0]["cls"] == A.TRIM_WHOLE).all()
    if name == "dovetail":
        assert A.TRIM_ENDS in lad.trims[0]["cls"].tolist()
    if name == "chimera_rc":
        assert lad.trims[0]["cls"][RF.CHIMERA] == A.TRIM_SPLIT
    if name == "chimera_rc_depth_only":
        assert lad.trims[0]["cls"][RF.CHIMERA] == A.TRIM_ENDS


# ---- the one-call routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_wrappers_equal_the_ladder(ctx, oracle, ladders, name):
    bases, offsets, params = case_batch(name)
    lad = ladders(name)
    host = wrappers(ctx, bases, offsets, params)
    equal_results(host, of_ladder(lad), name)
    assert host["read_chains"][0].dtype == np.dtype(A.CHAIN_DTYPE) and host["correct_trim_reads"][2].dtype == np.dtype(A.PILE_SEG_DTYPE)
    # longest: one segment per read, on the same table
    longest = RF.reference_tail(lad, params._replace(longest=True), oracle=oracle)
    best = minimizer.correct_trim_reads(ctx, bases, offsets, params.k, params.w, min_depth=params.min_depth, max_ins=params.max_ins,
                                        min_span=params.min_span, min_len=params.min_len, longest=True, band_chain=params.band_chain, band=params.band,
                                        max_trace_bytes=params.max_trace_bytes, **chain_kw(params))
    equal_results({"correct_trim_reads": best}, {"correct_trim_reads": of_ladder(longest)["correct_trim_reads"]}, name + " longest")
    assert len(best[2]) == int((lad.trims[0]["cls"] != A.TRIM_NONE).sum())
    # resident tensors: everything stays on the device and holds the same bytes
    dev = wrappers(ctx, *on_device(bases, offsets), params)
    assert all(x.is_cuda for res in dev.values() for x in res), name
    equal_results(dev, host, name + " on the device")
    # a second call on the same context
    equal_results(wrappers(ctx, bases, offsets, params), host, name + " again")


# ---- two batches ----------------------------------------------------------------------------------------------------------------------
def test_two_batches(ctx, oracle):
    q, db = (batch(x) for x in RF.two_batches())
    lad = device_ladder(ctx, *q, DEFAULT, *db)
    check_ladder(lad, oracle, DEFAULT, "q = dovetail, db = friendly and windows")
    assert len(lad.pile) == 2 and lad.pile[0] is not lad.pile[1] and len(lad.chains) >= 8 and set(lad.chains["read_b"].tolist()) == {1, 3, 5}
    assert (lad.chains["read_a"] == lad.chains["read_b"]).any() and lad.n_slots[0] + lad.n_slots[1] > 0
    hits = minimizer.chain_hits(ctx, lad.mini[0], lad.mini[1], upper=False)
    assert hits.tobytes() == lad.chains.tobytes()
    swapped = device_ladder(ctx, *db, DEFAULT, *q)
    check_ladder(swapped, oracle, DEFAULT, "q = friendly and windows, db = dovetail")
    RF.check_swapped(lad, swapped)


# ---- the route over its own output -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["friendly", "lower", "tandem", "identical"])
def test_second_round(ctx, oracle, ladders, name):
    """what correct_reads returns goes straight back in: the second round equals the reference ladder on the corrected batch"""
    _, _, p = case_batch(name)
    first = ladders(name)
    cons, cons_off = first.cons[0], first.cons_off[0]
    kw = dict(chain_kw(p), band_chain=p.band_chain, band=p.band, max_trace_bytes=p.max_trace_bytes, min_depth=p.min_depth, max_ins=p.max_ins)
    got = minimizer.correct_reads(ctx, cons, cons_off, p.k, p.w, **kw)
    want = RF.reference_ladder(oracle, cons, cons_off, p)
    assert len(want.chains) > 0
    for g, w, what in zip(got, (want.cons[0], want.cons_off[0], want.reads[0]), ("cons", "cons_offsets", "reads")):
        diff = RF.first_difference(g, w)
        assert diff is None, "%s, second round, %s: %s" % (name, what, diff)
    if name == "identical":
        assert raw(got[0]) == raw(first.bases) and raw(got[1]) == raw(first.offsets)
    if name == "lower":
        assert (cons != (cons & 0xDF)).any()   # a base without a call keeps the read's own lower-case byte, and goes in again as it is
    dev = minimizer.correct_reads(ctx, *on_device(cons, cons_off), p.k, p.w, **kw)
    assert all(x.is_cuda for x in dev) and [raw(x) for x in dev] == [raw(x) for x in got]


# ---- every family in one batch -------------------------------------------------------------------------------------------------------------
ALONE = ("tandem", "homopolymer", "identical", "palindrome", "unrelated", "dovetail", "chimera_rc")   # they share no sequence with the others


def test_families_in_one_batch(ctx, oracle):
    """all families in one batch at max_occ = 8: empty, short and chainless reads beside repeat-rich ones in the same tiles.  (The 24
    copies of the friendly template in friendly, edges and lower are above max_occ together: they seed nothing here.)"""
    p = DEFAULT._replace(max_occ=8)
    reads, first = [], {}
    for name, make in FAMILIES.items():
        first[name] = len(reads)
        reads += make()
    bases, offsets = batch(reads)
    lad = device_ladder(ctx, bases, offsets, p)
    check_ladder(lad, oracle, p, "all families")
    assert len(lad.chains) >= 60 and flag_counts(lad.aln)["chains"] == len(lad.chains)
    off, coff = offsets.astype(np.int64), lad.cons_off[0].astype(np.int64)
    for name in ALONE:
        mine = FAMILIES[name]()
        b, o = batch(mine)
        alone = device_ladder(ctx, b, o, p)
        r0, r1 = first[name], first[name] + len(mine)
        rows = slice(int(off[r0]), int(off[r1]))
        same_table(lad.pile[0][rows], alone.pile[0], name)
        assert lad.call[0][rows].tobytes() == alone.call[0].tobytes() and lad.ins_len[0][rows].tobytes() == alone.ins_len[0].tobytes(), name
        assert lad.reads[0][r0:r1].tobytes() == alone.reads[0].tobytes() and lad.trims[0][r0:r1].tobytes() == alone.trims[0].tobytes(), name
        assert lad.cons[0][int(coff[r0]):int(coff[r1])].tobytes() == alone.cons[0].tobytes(), name
        mine_chains = lad.chains[(lad.chains["read_a"] >= r0) & (lad.chains["read_a"] < r1)].copy()
        assert ((mine_chains["read_b"] >= r0) & (mine_chains["read_b"] < r1)).all(), name
        mine_chains["read_a"] -= r0
        mine_chains["read_b"] -= r0
        assert mine_chains.tobytes() == alone.chains.tobytes(), name


# ---- nothing to chain ------------------------------------------------------------------------------------------------------------------
EMPTY = {
    "read_chains": [(np.dtype(A.CHAIN_DTYPE), (0,))],
    "read_cigars": [(np.dtype(A.CHAIN_DTYPE), (0,)), (np.dtype(A.CHAIN_ALN_DTYPE), (0,)), (np.uint32, (0,)), (np.uint64, (1,))],
}


@pytest.mark.parametrize("reads", [FAMILIES["unrelated"](), ["", "", "", ""]], ids=["unrelated", "only_empty_reads"])
def test_no_chains_launches_cleanly(ctx, reads):
    """no chain at all, through every wrapper, on host and on resident arrays: every call returns, the results are empty or all
    zero with the dtypes and shapes of a full batch, and the stages behind the chaining still run their per-base kernels"""
    import torch
    bases, offsets = batch(reads)
    n_reads, n_bases = len(reads), int(offsets[-1])
    p = DEFAULT
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        host = wrappers(ctx, bases, offsets, p)
        ran = ctx.profile_get()
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    if n_bases:
        assert {"k_read_minimizers_count", "k_pile_call", "k_pile_reads", "k_cons_count", "k_seg_marks"} <= set(ran), sorted(ran)
        assert all(launches > 0 for launches, _ in ran.values())
    for name, shapes in EMPTY.items():
        for x, (dtype, shape) in zip(host[name], shapes):
            assert x.dtype == dtype and x.shape == shape, (name, x.dtype, x.shape)
    assert host["read_cigars"][3].tolist() == [0]
    chains, aln, pile, call, summary = host["read_pileups"]
    assert pile.dtype == np.uint32 and pile.shape == (n_bases, A.PILE_COLS) and not pile.any()
    assert call.dtype == np.uint8 and call.shape == (n_bases,) and (call == A.CALL_NONE).all()
    assert summary.dtype == np.dtype(A.READ_PILE_DTYPE) and summary.shape == (n_reads,) and summary["n_bases"].tolist() == [len(s) for s in reads]
    assert not summary["covered"].any() and not summary["depth_sum"].any()
    cons, cons_off, summary2 = host["correct_reads"]
    assert cons.dtype == np.uint8 and cons.tobytes() == bases.tobytes() and cons_off.dtype == np.uint64 and cons_off.tolist() == offsets.tolist()
    assert summary2.tobytes() == summary.tobytes()
    out, out_off, segs, summary3, trims = host["correct_trim_reads"]
    assert out.dtype == np.uint8 and out.shape == (0,) and out_off.dtype == np.uint64 and out_off.tolist() == [0]
    assert segs.dtype == np.dtype(A.PILE_SEG_DTYPE) and segs.shape == (0,) and summary3.tobytes() == summary.tobytes()
    assert trims.dtype == np.dtype(A.READ_TRIM_DTYPE) and trims.shape == (n_reads,) and (trims["cls"] == A.TRIM_NONE).all()
    assert trims["n_bases"].tolist() == [len(s) for s in reads]
    dev = wrappers(ctx, *on_device(bases, offsets), p)
    assert all(x.is_cuda for res in dev.values() for x in res)
    equal_results(dev, host, "on the device")
    assert tuple(dev["read_chains"][0].shape) == (0, 10) and dev["read_chains"][0].dtype == torch.int32
    assert tuple(dev["read_pileups"][2].shape) == (n_bases, A.PILE_COLS) and tuple(dev["correct_trim_reads"][2].shape) == (0, 4)

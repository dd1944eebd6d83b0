"""The three forms of a call -- host arrays, device tensors on a default context, device tensors on an async_device context
followed by synchronize() -- give the same bytes.  One small fixed-seed batch goes through every entry point whose host driver
is written in the shared steps of kmu_ctx.hpp (stage_to_device, place_output / bring_output, read_back, finish_*): read_minimizers,
read_anchors, anchor_match, anchor_overlaps, the anchor index's match, seed_chains, chain_align, chain_cigar, chain_pileup,
pile_call, pile_ins_plan, chain_pile_ins, pile_consensus, pile_consensus_pos, pile_segments, extract_ranges, sg_classify, sg_graph,
sig_knn, kmer_distribution, nthash, and of a counter query, once_positions, histogram and read_profile.  Beside the batch with a
non-empty result: one whose results are empty (total 0), and no reads at all (n == 0).  The count-then-write calls are also made
through the raw C-ABI with cap one below the total: KMU_E_BAD_ARG, and n_out is set all the same."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = {65: 84, 67: 71, 71: 67, 84: 65}
K, W = 15, 10


def overlapping_reads(seed, n_reads, length, root_len):
    """n_reads windows of one random sequence with 2 % substitutions and a few one-base gaps, every third one reverse-complemented"""
    rng = np.random.default_rng(seed)
    root = rng.choice(ACGT, root_len).astype(np.uint8)
    reads = []
    for r in range(n_reads):
        at = int(rng.integers(0, root_len - length + 1))
        s = root[at:at + length].copy()
        hit = rng.random(length) < 0.02
        s[hit] = rng.choice(ACGT, int(hit.sum()))
        s = np.delete(s, rng.integers(0, length, 3))
        s = np.insert(s, rng.integers(0, s.size, 3), rng.choice(ACGT, 3))
        if r % 3 == 2:
            s = np.array([COMP[int(b)] for b in s[::-1]], np.uint8)
        reads.append(s)
    offsets = np.zeros(n_reads + 1, np.uint64)
    offsets[1:] = np.cumsum([s.size for s in reads])
    return np.concatenate(reads), offsets


def unrelated_reads(seed, n_reads, length):
    """random reads that share nothing: no chain, no arc, no segment"""
    rng = np.random.default_rng(seed)
    offsets = (np.arange(n_reads + 1) * length).astype(np.uint64)
    return rng.choice(ACGT, n_reads * length).astype(np.uint8), offsets


def host(x):
    """what a call gave, as bytes: arrays and tensors by their bits, records of arrays in order, numbers as they are"""
    if x is None or isinstance(x, (int, np.integer)):
        return x
    if isinstance(x, (tuple, list)):
        return tuple(host(y) for y in x)
    if lib._is_torch(x):
        x = x.cpu().numpy()
    return np.ascontiguousarray(x).tobytes()


def by_value(values, mult, dist_off):
    """kmu_kmer_distribution leaves the distinct values of a read in no fixed order (two host calls differ as well): every
    read's (value, multiplicity) pairs sorted by value"""
    v, m, o = (np.frombuffer(host(x), t) for x, t in ((values, np.uint64), (mult, np.uint32), (dist_off, np.uint64)))
    order = np.concatenate([int(o[i]) + np.argsort(v[int(o[i]):int(o[i + 1])], kind="stable") for i in range(o.size - 1)] or
                           [np.zeros(0, np.int64)]).astype(np.int64)
    return v[order], m[order], o


def on_device(x):
    """a numpy array as a torch tensor on the device that holds the same bits"""
    import torch
    x = np.ascontiguousarray(x)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}.get(x.dtype)
    return torch.from_numpy((x.view(view) if view else x).copy()).cuda()


def route(ctx, bases, offsets, put):
    """every stage on the arrays as `put` places them (identity: host; on_device: device); the outputs by name"""
    out = {}
    n_reads = len(offsets) - 1
    b, off = put(bases), put(offsets)
    q = minimizer.read_minimizers(ctx, b, off, K, W)
    out["read_minimizers"] = (q.hashes, q.pos, q.read, q.strand, q.offsets)
    out["nthash"] = ctx.nthash(b, off, K, n_hashes=2)
    out["kmer_distribution"] = by_value(*ctx.kmer_distribution(b, off, A.KMER64BIT, K))
    p = A.SketchParams(A.ALGO_BOTTOMK, A.KMER64BIT, K, 8, A.SIG_U64, A.HASHER_INT64HASH, A.FHASH_CANON_VALUE, 0, A.MODE_PER_SEQ,
                       A.INPUT_ASCII, A.MEM_HOST, 0)
    hashes, counts, n, row_off = ctx.read_anchors(b, off, p, 200, 50)
    out["read_anchors"] = (hashes, counts, n, row_off)
    row_read = put((np.searchsorted(row_off, np.arange(int(row_off[-1])), side="right") - 1).astype(np.uint32))
    pairs, dist = ctx.anchor_match(hashes, hashes, n_keys=2, min_common=1, group_q=row_read, group_db=row_read)
    out["anchor_match"] = (pairs, dist)
    out["anchor_overlaps"] = ctx.anchor_overlaps(pairs, dist, row_off, strands=2, band=1, min_score=1)
    if hashes.shape[0]:
        out["sig_knn"] = ctx.sig_knn(hashes, hashes, 3, row_read, row_read)

    chains = minimizer.chain_hits(ctx, q, min_seeds=3)  # (the anchor index's match, then seed_chains)
    out["seed_chains"] = chains
    out["chain_align"] = ctx.chain_align(chains, b, off, band=64)
    aln, ops, op_off = out["chain_cigar"] = ctx.chain_cigar(chains, b, off, band=64)
    pile, _ = ctx.chain_pileup(chains, aln, ops, op_off, b, off)
    out["chain_pileup"] = pile
    call, reads = out["pile_call"] = ctx.pile_call(pile, b, off, min_depth=2)
    ins_len, n_slots = out["pile_ins_plan"] = ctx.pile_ins_plan(pile, call)
    ins, _ = ctx.chain_pile_ins(chains, aln, ops, op_off, b, off, ins_len, n_slots)
    out["chain_pile_ins"] = ins
    out["pile_consensus"] = ctx.pile_consensus(pile, call, ins_len, n_slots, ins, b, off)
    rows = put(np.arange(0, int(offsets[-1]), 37, dtype=np.uint64))
    out["pile_consensus_pos"] = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, b, off, rows)
    segs, seg_off, trims = out["pile_segments"] = ctx.pile_segments(pile, off, min_depth=2, min_len=50)
    out["pile_segments_longest"] = ctx.pile_segments(pile, off, min_depth=2, min_len=50, longest=True)
    first = np.asarray(offsets[:-1], np.uint64)
    out["extract_ranges"] = ctx.extract_ranges(b, put(first), put(first + np.minimum(np.diff(offsets), 100).astype(np.uint64)))
    out["sg_classify"] = ctx.sg_classify(chains, aln, off, min_overlap=200)
    out["sg_graph"] = ctx.sg_graph(chains, aln, off, min_overlap=200)

    with ctx.counter(A.KMER64BIT, 21, 8, 1 << 16) as c:
        c.add_reads(b, off)
        out["once_positions"] = c.once_positions(b, off)
        out["read_profile"] = c.read_profile(b, off)
        out["histogram"] = c.histogram(16, device=b.device if lib._is_torch(b) else None)
        out["query"] = c.query(out["once_positions"][0]) if n_reads else None
    ctx.synchronize()  # (an async_device context: the device calls above are in flight until here)
    return {name: host(v) for name, v in out.items()}


CASES = {
    "overlapping": lambda: overlapping_reads(0x5EED, 30, 900, 2400),  # chains, votes, slots, arcs: every result non-empty
    "unrelated": lambda: unrelated_reads(0x5EED, 24, 300),           # no chain: totals of 0 behind non-empty inputs
    "no_reads": lambda: (np.zeros(0, np.uint8), np.zeros(1, np.uint64)),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def forms(request):
    """(case, the outputs on host arrays, on device tensors, on device tensors of an async_device context)"""
    bases, offsets = CASES[request.param]()
    got = []
    for put, kw in ((lambda x: x, {}), (on_device, {}), (on_device, {"async_device": True})):
        ctx = lib.Context(0, **kw)
        try:
            got.append(route(ctx, bases, offsets, put))
        finally:
            ctx.close()
    return (request.param, bases, offsets) + tuple(got)


def test_device_calls_equal_host_calls(forms):
    _, _, _, want, dev, _ = forms
    assert sorted(dev) == sorted(want)
    differ = [name for name in want if dev[name] != want[name]]
    assert not differ, differ


def test_async_device_calls_equal_host_calls(forms):
    _, _, _, want, _, asy = forms
    assert sorted(asy) == sorted(want)
    differ = [name for name in want if asy[name] != want[name]]
    assert not differ, differ


def test_the_cases_reach_what_they_are_for(forms):
    name, bases, offsets, want = forms[:4]
    n_chains = len(want["seed_chains"]) // np.dtype(A.CHAIN_DTYPE).itemsize
    if name == "overlapping":
        assert n_chains >= 20 and len(want["chain_cigar"][1]) > 0 and len(want["anchor_match"][0]) > 0
        assert len(want["pile_segments"][0]) > 0 and len(want["sg_graph"][0]) > 0 and len(want["once_positions"][0]) > 0
        assert len(want["pile_consensus"][0]) > 0 and len(want["extract_ranges"][0]) == 30 * 100
    else:
        assert n_chains == 0 and len(want["chain_cigar"][1]) == 0 and len(want["pile_segments"][0]) == 0
        assert len(want["sg_graph"][0]) == 0
    if name == "no_reads":
        assert len(want["read_minimizers"][0]) == 0 and len(want["once_positions"][0]) == 0 and len(want["extract_ranges"][0]) == 0


# ---- count-then-write through the raw C-ABI: a capacity one below the total -----------------------------------------------------------
@pytest.fixture(scope="module")
def ctx():
    c = lib.Context(0)
    yield c
    c.close()


def vp(x):
    return lib._ptr(x)[0]


@pytest.mark.parametrize("put", [lambda x: x, on_device], ids=["host", "device"])
def test_a_capacity_one_below_the_total_is_refused_with_the_total(ctx, put):
    bases, offsets = overlapping_reads(7, 6, 400, 800)
    mem = A.MEM_HOST if put(bases) is bases else A.MEM_DEVICE
    n = C.c_uint64(0)

    # kmu_extract_ranges: 6 ranges of 50 bytes
    begin = np.asarray(offsets[:-1], np.uint64)
    b, lo, hi = put(bases), put(begin), put(begin + np.uint64(50))
    out_off, out = put(np.zeros(7, np.uint64)), put(np.zeros(300, np.uint8))
    rc = ctx.L.kmu_extract_ranges(ctx.h, vp(b), bases.size, vp(lo), vp(hi), 6, mem, vp(out_off), vp(out), 299, C.byref(n))
    assert rc == A.E_BAD_ARG and n.value == 300 and "cap = 299" in ctx.L.kmu_last_error(ctx.h).decode()
    assert ctx.L.kmu_extract_ranges(ctx.h, vp(b), bases.size, vp(lo), vp(hi), 6, mem, vp(out_off), vp(out), 300, C.byref(n)) == 0
    assert host(out) == b"".join(bases[int(s):int(s) + 50].tobytes() for s in begin)

    # kmu_pile_segments: every read is one supported segment
    pile = np.zeros((bases.size, A.PILE_COLS), np.uint32)
    pile[:, A.PILE_A] = 3
    p = A.PileSegParams(3, 0, 1, 0)
    d_pile, off = put(pile), put(offsets)
    seg_off, segs = put(np.zeros(7, np.uint64)), put(np.zeros(6 * 4, np.uint32))
    n.value = 0
    rc = ctx.L.kmu_pile_segments(ctx.h, vp(d_pile), vp(off), 6, C.byref(p), mem, vp(seg_off), vp(segs), 5, C.byref(n), None)
    assert rc == A.E_BAD_ARG and n.value == 6 and "cap = 5" in ctx.L.kmu_last_error(ctx.h).decode()
    assert ctx.L.kmu_pile_segments(ctx.h, vp(d_pile), vp(off), 6, C.byref(p), mem, vp(seg_off), vp(segs), 6, C.byref(n), None) == 0
    assert np.frombuffer(host(seg_off), np.uint64).tolist() == list(range(7))

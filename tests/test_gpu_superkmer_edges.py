"""Super-k-mer records (kmerutils_amd/csrc/kmu_smer.hip) where test_gpu_superkmer.py does not reach: units whose waves take more
than one step, owner counts on the LDS-atomic path and at the documented maximum, the shape of the records for every window form,
tiny and empty batches, device ranges `offsets + first` and what lies outside them, non-ACGT input, and the receiver fed with
records packed by hand.

The contract is the one of test_gpu_superkmer.py -- every canonical k-mer arrives once, at the owner the oracle names -- plus a
condition on the SHAPE of the records that follows from the format (superkmer_model.ideal_records): an owner never gets fewer
records than its runs of consecutive k-mers need at 16 k-mers a record, and all owners together get at most one more per wave-step
boundary (a step boundary cuts at most one run, a cut adds at most one record).  A sender that emitted a record per k-mer, or cut
runs anywhere else, fails it."""
import collections
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import superkmer_model as M
from kmerutils_amd import _abi as A
from kmerutils_amd import synth
from test_gpu_superkmer import _canon_kmers, _cases, _concat

pytestmark = pytest.mark.gpu

STEP_WORDS = 61               # SMER_STEP_WORDS: the 16-base words whose k-mers one wave step emits
STEP_BASES = STEP_WORDS * 16  # 976
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def dev(x):
    import torch
    return torch.from_numpy(x.astype(np.int64) if x.dtype == np.uint64 else x).cuda()


def rnd(rng, n):
    return bytes(ACGT[rng.integers(0, 4, n)])


class Side:
    """the oracle's side of one (batch, k): computed once, shared between the runs that need it, never changed"""

    def __init__(self, oracle, bases, off, k):
        self.want = _canon_kmers(oracle, bases, off, k)  # read order
        self.nk = np.maximum(np.diff(off.astype(np.int64)) - (k - 1), 0)
        assert self.want.size == int(self.nk.sum())


_INPUTS, _SIDES = {}, {}


def batch(name):
    if not _INPUTS:
        c = _cases()
        _INPUTS.update(ragged=c["ragged"], special=c["special"], one_long=c["one_long"], poly_a=_concat([b"A" * 500]))
    return _INPUTS[name]


def side_of(oracle, name, k):
    if (name, k) not in _SIDES:
        _SIDES[(name, k)] = Side(oracle, *batch(name), k)
    return _SIDES[(name, k)]


BIG = 1 << 20  # k-mers from which on the oracle side of a check is split over threads (the oracle's C calls and numpy's sort let go of the GIL)


def owners_of(O, kmers, k, n_parts):
    if kmers.size < BIG:
        return O.minimizer_owners(kmers, k, n_parts)
    with ThreadPoolExecutor(8) as pool:
        return np.concatenate(list(pool.map(lambda v: O.minimizer_owners(v, k, n_parts), np.array_split(kmers, 32))))


def expand_all(O, rec, k):
    """the canonical k-mers of the records, in record order, and whether every record is clean (oracle.superkmer_expand)"""
    if rec.shape[0] < BIG // 8:
        return O.superkmer_expand(rec, k)
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda r: O.superkmer_expand(r, k), np.array_split(rec, 32)))
    return np.concatenate([g for g, _ in parts]), all(c for _, c in parts)


def sorted_by_owner(kmers, owner, n_parts):
    """(the k-mers owner by owner, sorted within every owner; the first k-mer of every owner)"""
    out = kmers[np.argsort(owner.astype(np.uint16), kind="stable")]
    b = np.zeros(n_parts + 1, np.int64)
    b[1:] = np.cumsum(np.bincount(owner, minlength=n_parts))
    if out.size < BIG:
        for p in range(n_parts):
            out[b[p]:b[p + 1]].sort()
    else:
        with ThreadPoolExecutor(8) as pool:
            list(pool.map(lambda p: out[b[p]:b[p + 1]].sort(), range(n_parts)))
    return out, b


def check(ctx, bases, off, k, n_parts, mem, side=None, reads=None, dev_in=None):
    """extract_superkmers of reads [first, last) of the batch (all of them by default) against the oracle and the model; mem: "dev" or
    "host" (dev_in: the batch already on the device).  Returns the records per owner."""
    from oracle import oracle as O
    first, last = reads if reads else (0, off.size - 1)
    b0, b1 = int(off[first]), int(off[last])
    if side is None:
        sub = np.ascontiguousarray(bases[b0:b1]) if b1 > b0 else np.zeros(1, np.uint8)
        side = Side(O, sub, off[first:last + 1] - off[first], k)
    c = ctx.counter(A.KMER64BIT, k, 16, 1 << 16)
    if mem == "dev":
        db, do = dev_in if dev_in else (dev(bases), dev(off))
        rec, bounds, kmers = c.extract_superkmers(db, do[first:last + 1], n_parts)
        origin = b0 & ~1023  # the walk of a device range starts at the 1024-base step that holds its first base ...
    else:
        rec, bounds, kmers = c.extract_superkmers(bases, np.ascontiguousarray(off[first:last + 1]), n_parts)
        origin = b0          # ... host input is staged from its first base on
    ctx.synchronize()
    rec = rec.cpu().numpy().view(np.uint32).reshape(-1, 3)
    c.close()
    what = (k, n_parts, mem, reads)
    # 1. totals
    bounds, kmers = bounds.astype(np.int64), kmers.astype(np.int64)
    assert bounds[0] == 0 and int(bounds[-1]) == rec.shape[0] and int(kmers.sum()) == side.want.size, what
    records = np.diff(bounds)
    assert (records >= 0).all(), what
    # 2. per owner: the records expand cleanly into kmers[p] k-mers, all of owner p, and sorted they are the oracle's k-mers of owner p.
    # Every owner at once: the expansion keeps the order of the records, so a k-mer's group is that of its record.
    got, clean = expand_all(O, rec, k)
    assert clean, "a record carries bits behind its last base: %s" % (what,)
    group = np.repeat(np.repeat(np.arange(n_parts), records), (rec[:, 2] & 15).astype(np.int64) + 1)
    assert got.size == group.size and np.array_equal(np.bincount(group, minlength=n_parts), kmers), what
    if got.size < BIG:  # (said outright where it is cheap.  It follows from the comparison below: equal k-mers have equal owners, and the
        #  oracle's k-mers stand in the group of their owner)
        assert np.array_equal(O.minimizer_owners(got, k, n_parts), group), what
    own = owners_of(O, side.want, k, n_parts).astype(np.int64)  # read order
    got_sorted, got_first = sorted_by_owner(got, group, n_parts)
    want_sorted, want_first = sorted_by_owner(side.want, own, n_parts)
    assert np.array_equal(got_first, want_first) and np.array_equal(got_sorted, want_sorted), what
    # 3. record shape
    ideal = M.ideal_records(own, side.nk, n_parts)
    nwords = -(-(b1 - origin) // 16)
    nsteps = -(-nwords // STEP_WORDS)
    assert (records >= ideal).all(), (what, records, ideal)
    assert int(records.sum()) <= int(ideal.sum()) + max(nsteps - 1, 0), (what, int(records.sum()), int(ideal.sum()), nsteps)
    return records


# ---- units whose waves take a second step ------------------------------------------------------------------------------------
_BIG = {}


def multi_step_reads():
    """ONT-shaped reads of just above (8 * 8 * CUs + 1) * 976 bases: smer_units (kmu_smer.hip) gives 8 * CUs units of
    steps_per_unit = 9, so that every one of a unit's four waves takes at least two steps and wave 0 three.  Mirrors smer_units."""
    if "reads" not in _BIG:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        need = (8 * 8 * cus + 1) * STEP_BASES + 7
        rng = np.random.default_rng(0xB16)
        lens = synth.ont_lengths(need // 2000, rng)
        cut = int(np.searchsorted(np.cumsum(lens), need))
        lens = lens[:cut + 1].copy()
        lens[-1] -= int(lens.sum()) - need
        bases, off = synth.genome_reads(lens.size, lens, 3_000_000, 0xB17, sub=0.04, ins=0.02, dele=0.02)
        nsteps = -(-(-(-int(off[-1]) // 16)) // STEP_WORDS)
        units = min(nsteps, 8 * cus)
        assert int(off[-1]) == need and -(-nsteps // units) >= 9
        _BIG["reads"] = (bases, off, dev(bases), dev(off))
    return _BIG["reads"]


@pytest.mark.parametrize("k,n_parts", [(31, 8), (31, 13), (21, 6)])
def test_units_of_several_steps_per_wave(ctx, oracle, k, n_parts):
    bases, off, db, do = multi_step_reads()
    if ("side", k) not in _BIG:
        _BIG[("side", k)] = Side(oracle, bases, off, k)
    records = check(ctx, bases, off, k, n_parts, "dev", side=_BIG[("side", k)], dev_in=(db, do))
    assert (records > 0).all()


# ---- owner counts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_parts", [9, 16, 2048])
@pytest.mark.parametrize("k", [31, 24, 17])
def test_owner_counts_behind_the_packed_path(ctx, oracle, k, n_parts):
    """9: the first count on the LDS-atomic path; 16: a power of two there (the mask); 2048: the documented maximum"""
    for name in ("ragged", "special"):
        bases, off = batch(name)
        for mem in ("dev", "host"):
            check(ctx, bases, off, k, n_parts, mem, side=side_of(oracle, name, k))


@pytest.mark.parametrize("n_parts", [0, 2049])
def test_owner_counts_out_of_range_are_refused(ctx, oracle, n_parts):
    from kmerutils_amd import lib
    bases, off = batch("ragged")
    c = ctx.counter(A.KMER64BIT, 31, 16, 1 << 16)
    ctx.profile_reset()
    ctx.profile_enable(True)
    try:
        for b, o in ((bases, off), (dev(bases), dev(off))):
            with pytest.raises(lib.KmuError) as e:
                c.extract_superkmers(b, o, n_parts)
            assert e.value.code == A.E_BAD_ARG
        ctx.synchronize()
        assert not [name for name in ctx.profile_get() if name.startswith("k_smer")]  # refused before any kernel of the sender ran ...
        c.extract_superkmers(bases, off, 8)
        ctx.synchronize()
        assert {"k_smer_census", "k_smer_scatter"} <= set(ctx.profile_get())  # ... which the profile would have shown
    finally:
        ctx.profile_enable(False)
        ctx.profile_reset()
    c.close()
    check(ctx, bases, off, 31, 8, "dev", side=side_of(oracle, "ragged", 31))  # the context is as good as before


# ---- record shape for every window form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_parts", [1, 8, 13])
@pytest.mark.parametrize("k", [31, 29, 28, 24, 23, 17])
def test_record_shape_of_every_window_form(ctx, oracle, k, n_parts):
    """W = 21 (k = 29 .. 31), W = 16 (24 .. 28) and W = 9 (17 .. 23) at both ends of their ranges; 1 and 8 owners on the packed path,
    13 on the other"""
    for name in ("one_long", "ragged", "poly_a"):
        bases, off = batch(name)
        side = side_of(oracle, name, k)
        for mem in ("dev", "host"):
            records = check(ctx, bases, off, k, n_parts, mem, side=side)
            if n_parts == 1 and int(off[-1]) <= STEP_BASES:  # one owner, one step: a read of n k-mers is exactly ceil(n / 16) records
                assert int(records[0]) == int(((side.nk + 15) // 16).sum())


# ---- tiny and empty batches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 24, 17])
def test_tiny_and_empty_batches(ctx, oracle, k):
    rng = np.random.default_rng(100 + k)
    cases = [[], [b"", b"", b""], [rnd(rng, k), rnd(rng, k)]] + [[rnd(rng, n)] for n in (k - 1, k, 15, 16, 17)]
    for seqs in cases:
        bases, off = _concat(seqs)
        n_kmers = sum(max(len(s) - k + 1, 0) for s in seqs)
        side = Side(oracle, bases, off, k)
        assert side.want.size == n_kmers
        for n_parts in (8, 9):
            for mem in ("dev", "host"):
                records = check(ctx, bases, off, k, n_parts, mem, side=side)
                assert int(records.sum()) == min(n_kmers, len(seqs))  # no k-mer: no record, all bounds zero; one k-mer per read: one record each


# ---- ranges of a larger read set ----------------------------------------------------------------------------------------------
# where the first read of a range starts: a step edge of the 976-base walk and one word past it, the edge of the 1024-base re-basing
# of device ranges and mid-step; the same 2 048 bases on, where a byte 1 500 bases before the range exists
FIRST_AT = [975, 976, 992, 1023, 1024, 2000, 3023, 3071, 3072]
_RANGE = {}


def range_reads():
    if not _RANGE:
        rng = np.random.default_rng(0xA11)
        lens = np.diff([0] + FIRST_AT).tolist() + [300, 17, 1201, 40, 2500, 5]
        seqs = [rnd(rng, n) for n in lens]
        bases, off = _concat(seqs)
        assert set(FIRST_AT) <= set(int(v) for v in off)
        _RANGE["r"] = (bases, off)
    return _RANGE["r"]


def first_at(off, pos):
    return int(np.flatnonzero(off == pos)[0])


@pytest.mark.parametrize("k", [31, 24, 17])
def test_device_and_host_ranges(ctx, oracle, k):
    bases, off = range_reads()
    n = off.size - 1
    dev_in = (dev(bases), dev(off))
    for pos in FIRST_AT:
        first = first_at(off, pos)
        for last in (n, n - 2, first + 1, first):
            for mem in ("dev", "host"):
                check(ctx, bases, off, k, 8, mem, reads=(first, last), dev_in=dev_in)
        check(ctx, bases, off, k, 13, "dev", reads=(first, n), dev_in=dev_in)


def dump_of(ctx, k, bases, off, path):
    c = ctx.counter(A.KMER64BIT, k, 16, (1 << 23) if path == "single_pass" else (1 << 14))
    c.add_reads(bases, off)
    got = c.dump(1)
    c.close()
    return got


PATHS = {"default": {}, "direct": {"KMU_COUNT_PATH": "direct"}, "partitioned": {"KMU_COUNT_PATH": "partitioned"},
         "single_pass": {"KMU_COUNT_PATH": "partitioned", "KMU_COUNT_SEG": "2"}}  # (the last: k_part_scatter1 on a two-level table)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("k", [31, 17])
def test_bases_outside_a_range_are_not_the_calls(ctx, oracle, monkeypatch, k, path):
    """One non-ACGT byte in a read BEFORE the range -- 10 bases before its first base, which a device range's walk passes wherever
    the range does not start on a multiple of 1 024, and 1 500 bases before it -- or in a read BEHIND it: the call succeeds and
    computes what the oracle computes on the reads of the range, for extract_superkmers and for add_reads, from device and from host
    memory.  Whether a call succeeds does not depend on where its range sits in the 1 024-base grid."""
    for name, value in PATHS[path].items():
        monkeypatch.setenv(name, value)
    clean, off = range_reads()
    n = off.size - 1
    for pos in FIRST_AT:
        first = first_at(off, pos)
        for last, at in [(n, pos - 10), (n - 2, pos - 10), (n - 2, int(off[n - 2]) + 3)] + ([(n, pos - 1500)] if pos >= 1500 else []):
            bases = clean.copy()
            bases[at] = ord("N")
            sub_b, sub_o = np.ascontiguousarray(bases[pos:int(off[last])]), off[first:last + 1] - off[first]
            o = oracle.Counter(A.KMER64BIT, k, 16, 1 << 14)
            o.add_reads(sub_b, sub_o)
            wk, wc = o.dump(1)
            dev_in = (dev(bases), dev(off))
            for mem in ("dev", "host"):
                if path == "default":
                    check(ctx, bases, off, k, 8, mem, reads=(first, last), dev_in=dev_in)
                b, o_ = (dev_in[0], dev_in[1][first:last + 1]) if mem == "dev" else (bases, np.ascontiguousarray(off[first:last + 1]))
                gk, gc = dump_of(ctx, k, b, o_, path)
                assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (k, path, pos, last, at, mem)


# ---- non-ACGT bytes inside the batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 17])
def test_non_acgt_inside_the_batch_is_refused_and_forgotten(ctx, oracle, k):
    from kmerutils_amd import lib
    rng = np.random.default_rng(0xBAD + k)
    seqs = [rnd(rng, 500), rnd(rng, 12), rnd(rng, 600), rnd(rng, 2 * STEP_BASES + 300 + 7 - 1112)]
    clean, off = _concat(seqs)
    total = int(off[-1])
    assert total % 16 == 3 and total > 2 * STEP_BASES
    side = Side(oracle, clean, off, k)
    spots = {"a lane's own word mid-step": 16 * 30 + 5, "the halo of step 0 (word 62), step 1's own": 16 * 62 + 4,
             "the last, partial word of the stream": total - 2, "a read shorter than k": 505}
    for what, at in spots.items():
        bases = clean.copy()
        bases[at] = ord("N")
        for mem in ("dev", "host"):
            b, o = (dev(bases), dev(off)) if mem == "dev" else (bases, off)
            raised = []
            for call in ("extract_superkmers", "add_reads"):
                c = ctx.counter(A.KMER64BIT, k, 16, 1 << 14)
                try:
                    c.extract_superkmers(b, o, 8) if call == "extract_superkmers" else c.add_reads(b, o)
                    ctx.synchronize()
                    raised.append(False)
                except lib.KmuError as e:
                    assert e.code == A.E_NON_ACGT, (what, mem, call)
                    raised.append(True)
                c.close()
            # extract_superkmers refuses a batch if and only if add_reads refuses it; both do wherever the byte lies in a read
            assert raised == [True, True], (what, mem, raised)
            check(ctx, clean, off, k, 8, mem, side=side)  # the error word does not leak into the next call
    lower = clean.copy()
    lower[100:1500] = np.frombuffer(lower[100:1500].tobytes().lower(), np.uint8)  # lower case letters are bases
    for mem in ("dev", "host"):
        check(ctx, lower, off, k, 8, mem, side=side)


# ---- the receiver, on records packed by hand ----------------------------------------------------------------------------------
_GENOME = np.random.default_rng(0x6E0).choice(ACGT, size=2000).tobytes()
_RC = bytes.maketrans(b"ACGT", b"TGCA")
_HAND = {}


def hand_records(n, k, lengths):
    """n records from either strand of a 2 000-base genome (so that k-mers occur more than once), record i holding lengths[i % len]
    k-mers; the expected counts from the bases of every record, with the model alone"""
    if (n, k, lengths) not in _HAND:
        rng = np.random.default_rng(n * 64 + k)
        rec = np.zeros((n, 3), np.uint32)
        cnt = collections.Counter()
        for i in range(n):
            nb = lengths[i % len(lengths)] + k - 1
            s = int(rng.integers(0, len(_GENOME) - nb + 1))
            b = _GENOME[s:s + nb]
            if i & 1:
                b = b[::-1].translate(_RC)
            rec[i] = M.pack_record(b, k)
            cnt.update(M.canon_kmers(b, k).tolist())
        keys = np.array(sorted(cnt), np.uint64)
        _HAND[(n, k, lengths)] = (rec, keys, np.array([cnt[int(x)] for x in keys], np.uint32))
    return _HAND[(n, k, lengths)]


@pytest.mark.parametrize("path", [None, "direct", "partitioned"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_receiver_counts_hand_packed_records(ctx, monkeypatch, path, n):
    """k_smer_count_kmers, k_smer_expand and k_smer_scatter1 without the sender: record counts around the wave (64) and the
    workgroup (256), idle lanes in the last wave; the largest record of the format (16 k-mers at k = 31: 92 of the 96 bits) and the
    smallest (one k-mer at k = 17)"""
    import torch
    if path:
        monkeypatch.setenv("KMU_COUNT_PATH", path)
    if path == "partitioned":  # (as test_gpu_superkmer.py: the single-pass partition whatever the batch size, on a two-level table)
        monkeypatch.setenv("KMU_COUNT_SEG", "2")
    for k, lengths in ((31, (1, 16, 7, 2)), (17, (1, 16, 7, 2)), (31, (16,)), (17, (1,)), (24, (16, 1))):
        rec, wk, wc = hand_records(n, k, lengths)
        assert n < 4097 or wc.max() > 1
        for mem_dev in (True, False):
            c = ctx.counter(A.KMER64BIT, k, 16, (1 << 23) if path == "partitioned" else 1 << 14)
            for times in (1, 2):  # the same records a second time double every count
                c.add_superkmers(torch.from_numpy(rec.view(np.int32)).cuda() if mem_dev else rec)
                gk, gc = c.dump(1)
                order = np.argsort(gk, kind="stable")
                assert np.array_equal(gk[order], wk) and np.array_equal(gc[order], times * wc), (n, k, lengths, path, mem_dev, times)
            c.close()

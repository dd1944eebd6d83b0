"""k_sketch_super (kmerutils_amd/csrc/kmu_sketch_super.hip) where the other files do not reach: on the thresholds of its launch plan
(super_plan, kmu_sketch_host.hpp), with reads on the edges of its staging chunk (512 items) and of a batch (ncol items), reads that
start at every offset inside a 16-base word, a workgroup that takes a second and a third read, pre-hashed lists, the all-sequences
path over several chunks and reduce blocks, and one context that changes plans from call to call.

The plan for a staging chunk of 512 items and 160 KiB of LDS (tests/cpp/test_super_plan.cpp pins it):

    m      entry  threads  ncol  lds (bytes)               blocks/CU
    2      u8     256      256   4 656                     8
    225    u8     256      256   65 312 (no attribute)     2
    226    u8     256      256   65 584 (attribute call)   2
    256    u8     256      256   73 744                    2
    257    u16    256      256   139 808                   1
    302    u16    256      256   163 568                   1
    303    u16    192      192   125 312                   1
    399    u16    192      192   163 712                   1
    400    u16    128      128   112 912                   1
    587    u16    128      128   163 776                   1
    588    u16    64       64    88 784                    1
    1109   u16    64       64    163 808                   1
    1110   u16    64       63    <= 163 840                1
    2500   u16    64       23                              1
    8872   u16    64       1                               1
    8873   refused (KMU_E_UNSUPPORTED)

Every comparison is bit for bit on the whole signature array against the CPU oracle (oracle/kmu_oracle.c), which restates the
sequential algorithm with its exact a_upper histogram."""
import time

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

pytestmark = pytest.mark.gpu

K = 21
# m -> ncol of the table above
NCOL = {2: 256, 3: 256, 225: 256, 226: 256, 256: 256, 257: 256, 302: 256, 303: 192, 399: 192, 400: 128, 587: 128, 588: 64, 1109: 64,
        1110: 63}
PLAN_M = sorted(NCOL)
BOTH_FLAGS_M = (256, 257, 302, 303, 1109, 1110)  # all four forms, with and without FLAG_RAND08
FORMS = {"f64": (A.ALGO_SUPER, A.SIG_F64), "f32": (A.ALGO_SUPER, A.SIG_F32), "u64": (A.ALGO_SUPER2, A.SIG_U64),
         "u32": (A.ALGO_SUPER2, A.SIG_U32)}
DNA_FH = A.FHASH_CANON_INVHASH


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def n_cus():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def params(form, m, hasher=A.HASHER_NOHASH, flags=0, kmer_type=A.KMER64BIT, k=K, fhash=DNA_FH, mode=A.MODE_PER_SEQ, kind=A.INPUT_ASCII):
    algo, sig = FORMS[form]
    return A.SketchParams(algo, kmer_type, k, m, sig, hasher, fhash, 0, mode, kind, 0, flags)


def dna(rng, n):
    return bytes(synth.ACGT[rng.integers(0, 4, n)])


def reads_of_nk(rng, nks, k=K):
    """one random read per entry of nks with that many k-mers (0: a read of k - 1 bases)"""
    return [dna(rng, nk + k - 1) for nk in nks]


def same_bits(got, want, what=""):
    got = np.asarray(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        rows = np.nonzero((got.reshape(want.shape[0], -1).view(np.uint8) != want.reshape(want.shape[0], -1).view(np.uint8)).any(axis=1))[0]
        raise AssertionError("%s: rows differ from the oracle: %s" % (what, rows[:10].tolist()))


def from_device(t, want):
    return t.cpu().numpy().view(want.dtype)


# ---- a. the thresholds of the plan -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", PLAN_M)
def test_plan_edges(ctx, oracle, m):
    """reads of 0, 1, 2 k-mers, one batch (ncol) minus one / exactly / plus one, and the staging chunk's 511 / 512 / 513, 1024 / 1025
    and 1537, at every m on a threshold of the plan"""
    ncol = NCOL[m]
    nks = sorted({0, 1, 2, ncol - 1, ncol, ncol + 1, 511, 512, 513, 1024, 1025, 1537})
    bases, off = oracle.concat(reads_of_nk(np.random.default_rng(7000 + m), nks))
    i = PLAN_M.index(m)
    if m in BOTH_FLAGS_M:
        # a form meets one hasher without the flag and the other with it; which is which alternates from m to m
        cases = [(form, flags, (A.HASHER_NOHASH, A.HASHER_FNV1A)[(i + (flags != 0)) % 2]) for form in FORMS for flags in (0, A.FLAG_RAND08)]
    else:
        cases = [("f64", 0, (A.HASHER_NOHASH, A.HASHER_FNV1A)[i % 2]), ("u64", 0, (A.HASHER_FNV1A, A.HASHER_NOHASH)[i % 2])]
    for form, flags, hasher in cases:
        p = params(form, m, hasher, flags)
        same_bits(ctx.sketch(bases, off, p), oracle.sketch(bases, off, p), "m %d %s flags %d hasher %d" % (m, form, flags, hasher))


# ---- b. one wave, few item lanes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2500, 8872])
@pytest.mark.parametrize("form", ["f32", "u64"])
def test_one_wave_few_columns(ctx, oracle, m, form):
    """ncol = 23 and ncol = 1: reads on either side of one and two batches of 23, and one longer than the staging chunk.  f32 at
    these m: r + j is rounded to 2^-13 .. 2^-11 and the bound is the floor of such values"""
    bases, off = oracle.concat(reads_of_nk(np.random.default_rng(7100 + m), [1, 2, 22, 23, 24, 47, 600]))
    p = params(form, m, A.HASHER_FNV1A if form == "f32" else A.HASHER_NOHASH)
    want = oracle.sketch(bases, off, p)
    ctx.synchronize()
    t0 = time.perf_counter()
    got = ctx.sketch(bases, off, p)
    dt = time.perf_counter() - t0
    print("one wave, m = %d, %s: %.1f ms for 7 reads" % (m, form, dt * 1e3))
    same_bits(got, want, "m %d %s" % (m, form))


# ---- c. the refusal ---------------------------------------------------------------------------------------------------------
def test_refused_above_8872(ctx, oracle):
    """m >= 8873: not even one permutation column fits beside the slots -- KMU_E_UNSUPPORTED before any launch, for sequences, for
    pre-hashed values and in the all-sequences mode, and the context goes on working"""
    from kmerutils_amd.lib import KmuError
    bases, off = oracle.concat(reads_of_nk(np.random.default_rng(7200), [0, 1, 70, 600]))
    vals = np.arange(100, dtype=np.uint64)
    voff = np.array([0, 40, 100], np.uint64)
    for m in (8873, 65536):
        for form in ("f64", "f32", "u64", "u32"):
            with pytest.raises(KmuError) as e:
                ctx.sketch(bases, off, params(form, m))
            assert e.value.code == A.E_UNSUPPORTED, (m, form)
        for mode in (A.MODE_PER_SEQ, A.MODE_ALL_SEQS):
            with pytest.raises(KmuError) as e:
                ctx.sketch_hashed(vals, voff, params("u64", m, mode=mode))
            assert e.value.code == A.E_UNSUPPORTED, (m, mode)
        with pytest.raises(KmuError) as e:
            ctx.sketch(bases, off, params("f64", m, mode=A.MODE_ALL_SEQS))
        assert e.value.code == A.E_UNSUPPORTED, m
    for form in ("f64", "u64"):
        p = params(form, 64)
        same_bits(ctx.sketch(bases, off, p), oracle.sketch(bases, off, p), "m 64 after a refusal, %s" % form)
    p = params("u32", 8872)  # the largest sketch is not refused
    same_bits(ctx.sketch(bases[:int(off[3])], off[:4], p), oracle.sketch(bases[:int(off[3])], off[:4], p), "m 8872")


# ---- d. a workgroup's second and third read --------------------------------------------------------------------------------
def _short_reads(oracle, seed, n):
    """n reads of 21 .. 90 bases; every fifth has no k-mer (20 bases) and every fifth, two places on, a single one: whichever of them
    a workgroup takes after a full read shows slots or a bound left over from that read"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(K, 91, n)
    lens[0::5] = K - 1
    lens[2::5] = K
    return oracle.concat([dna(rng, int(L)) for L in lens])


@pytest.mark.parametrize("m,form,per_cu", [(64, "f32", 8), (300, "u32", 1), (1110, "u64", 1)])
def test_workgroup_takes_a_third_read(ctx, oracle, n_cus, m, form, per_cu):
    """more than twice as many reads as the grid has workgroups (at most per_cu per CU): some workgroup takes three, and resets its
    slots, its bound and its queue word between them"""
    bases, off = _short_reads(oracle, 7300 + m, 2 * per_cu * n_cus + 17)
    p = params(form, m, A.HASHER_FNV1A if m == 300 else A.HASHER_NOHASH)
    same_bits(ctx.sketch(bases, off, p), oracle.sketch(bases, off, p), "m %d %s" % (m, form))


# ---- e. where a read starts -------------------------------------------------------------------------------------------------
def _reads_at_lead(rng, lead, nks, packed):
    """reads of nks k-mers, each behind a pad read whose length puts the read's first base `lead` bases into a 16-base word of the
    batch (ASCII: byte offset mod 16; packed: every read starts a byte, (byte offset mod 4) * 4).  -> (reads, indices of the placed ones)"""
    seqs, placed, cur = [], [], 0  # cur: bases (ASCII) or bytes (packed) so far
    for nk in nks:
        if packed:
            pad = 4 * (6 + (lead // 4 - (cur + 6)) % 4)
            cur += pad // 4
        else:
            pad = K + (lead - (cur + K)) % 16
            cur += pad
        seqs.append(dna(rng, pad))
        L = nk + K - 1
        placed.append(len(seqs))
        seqs.append(dna(rng, L))
        cur += (L + 3) // 4 if packed else L
    return seqs, placed


def _lead_nks(lead):
    return [1024 - lead - 1, 1024 - lead, 1024 - lead + 1, 1536]


def _second_step_matters(oracle, read, lead, p):
    """True if the oracle's signature of `read` needs the k-mers at 1024 - lead .. 1023: those of its second chunk (512 .. 1023) that
    lie in the second wave-step of its words, which a step bound that forgets `lead` leaves out.  At m = 64 most of 1 536 k-mers
    hold no slot, and a sketch that skips a few of them is still right by luck; the tests below also sketch at an m where it is not"""
    bases, off = oracle.concat([read])
    vals = oracle.kmer_hashes(bases, off, p.kmer_type, p.kmer_size, p.fhash)[:len(read) - p.kmer_size + 1]
    rest = np.delete(vals, np.arange(1024 - lead, 1024))

    def one(v):
        return oracle.sketch_hashed(v, np.array([0, v.size], np.uint64), p)
    assert one(vals).tobytes() == oracle.sketch(bases, off, p).tobytes()
    return one(rest).tobytes() != one(vals).tobytes()


@pytest.mark.parametrize("lead", range(16))
def test_read_start_ascii(ctx, oracle, lead):
    """a read whose k-mers end one short of, on and one past the first wave-step (1 024 bases of the words the read lies in), and one
    whose second chunk ends inside the second step, from every start inside a word"""
    seqs, placed = _reads_at_lead(np.random.default_rng(7400 + lead), lead, _lead_nks(lead), False)
    bases, off = oracle.concat(seqs)
    assert all(int(off[i]) % 16 == lead for i in placed)
    assert lead == 0 or _second_step_matters(oracle, seqs[placed[3]], lead, params("f64", 2500))
    for m in (64, 2500):
        p = params("f64", m)
        same_bits(ctx.sketch(bases, off, p), oracle.sketch(bases, off, p), "lead %d m %d" % (lead, m))


@pytest.mark.parametrize("lead", [0, 4, 8, 12])
def test_read_start_packed(ctx, oracle, lead):
    """the same with 2-bit packed reads: four bases a byte, a read starts a byte"""
    seqs, placed = _reads_at_lead(np.random.default_rng(7450 + lead), lead, _lead_nks(lead), True)
    bases, off = oracle.concat(seqs)
    packed, poff = ctx.pack2b(bases, off)
    assert all(int(poff[i]) % 4 == lead // 4 for i in placed)
    assert all(bytes(packed[int(poff[i]):int(poff[i + 1])]) == bytes(oracle.pack2b(seqs[i])) for i in placed)
    assert lead == 0 or _second_step_matters(oracle, seqs[placed[3]], lead, params("u32", 2500))
    for form, m in (("f64", 64), ("u32", 64), ("u32", 2500)):
        want = oracle.sketch(bases, off, params(form, m))
        same_bits(ctx.sketch(packed, off, params(form, m, kind=A.INPUT_PACKED2), packed_offsets=poff), want,
                  "packed lead %d %s m %d" % (lead, form, m))


@pytest.mark.parametrize("nk", [512, 1024, 1536])
def test_non_acgt_in_the_tail_words(ctx, oracle, nk):
    """a read whose k-mers fill its chunks exactly: the last k - 1 bases start no k-mer, and in the last 15 of them a byte that is no
    base must still be seen -- the last chunk walks the words that hold only the tail"""
    from kmerutils_amd.lib import KmuError
    rng = np.random.default_rng(7500 + nk)
    p = params("f64", 64)
    for lead, back in ((0, 1), (0, 15), (5, 1), (12, 8), (15, 15)):
        pad, read = dna(rng, 32 + lead), bytearray(dna(rng, nk + K - 1))
        clean, off = oracle.concat([pad, bytes(read)])
        same_bits(ctx.sketch(clean, off, p), oracle.sketch(clean, off, p), "nk %d lead %d" % (nk, lead))
        read[-back] = ord("N")
        bases, off = oracle.concat([pad, bytes(read)])
        with pytest.raises(KmuError) as e:
            ctx.sketch(bases, off, p)
        assert e.value.code == A.E_NON_ACGT, (nk, lead, back)
        with pytest.raises(oracle.OracleError):
            oracle.sketch(bases, off, p)


# ---- f. amino acids ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kmer_type,k", [(A.KMERAA64BIT, 12), (A.KMERAA32BIT, 5)])
def test_amino_acid_chunk_edges(ctx, oracle, kmer_type, k):
    """the amino-acid walk stages 64 positions a wave-step: sequences on that edge and on the staging chunk's"""
    rng = np.random.default_rng(7600 + k)
    seqs = [bytes(synth.AA20[rng.integers(0, 20, nk + k - 1)]) for nk in (63, 64, 65, 511, 512, 513, 1025)]
    res, off = oracle.concat(seqs)
    for form, m, hasher in (("f64", 128, A.HASHER_NOHASH), ("f32", 303, A.HASHER_FNV1A)):
        p = params(form, m, hasher, kmer_type=kmer_type, k=k, fhash=A.FHASH_VALUE_MASKED)
        same_bits(ctx.sketch(res, off, p), oracle.sketch(res, off, p), "aa k %d m %d %s" % (k, m, form))


# ---- g. pre-hashed lists ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt,kmer_type,k", [(np.uint64, A.KMER64BIT, 21), (np.uint32, A.KMER16B32BIT, 16)])
@pytest.mark.parametrize("m", [257, 1110])
def test_hashed_lists(ctx, oracle, dt, kmer_type, k, m):
    """lists of 0, 1, 512, 513 and 5 000 values, empty ones between full ones; from the host, and from device memory where the first
    list does not start at value 0"""
    import torch
    rng = np.random.default_rng(7700 + m)
    lens = [0, 1, 0, 512, 513, 0, 0, 5000, 0]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    vals = rng.integers(0, 2**32 if dt == np.uint32 else 2**63, int(off[-1]), dtype=np.uint64).astype(dt)
    vals[600:700] = vals[600]  # repeats
    skip = 37
    shifted = np.concatenate([rng.integers(0, 2**31, skip, dtype=np.uint64).astype(dt), vals])
    d_vals = torch.from_numpy(shifted.view(np.int32 if dt == np.uint32 else np.int64)).cuda()
    d_off = torch.from_numpy((off + np.uint64(skip)).astype(np.int64)).cuda()
    for form, hasher in (("f64", A.HASHER_FNV1A), ("u32", A.HASHER_NOHASH)):
        p = params(form, m, hasher, kmer_type=kmer_type, k=k, fhash=0)
        want = oracle.sketch_hashed(vals, off, p)
        same_bits(ctx.sketch_hashed(vals, off, p), want, "host m %d %s" % (m, form))
        same_bits(from_device(ctx.sketch_hashed(d_vals, d_off, p), want), want, "device m %d %s" % (m, form))


# ---- h. all sequences -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def all_seqs_batch(oracle):
    """reads with 32 769 k-mers in all; the first 6 hold 16 384 and the first 7 hold 16 385 (one read of a single k-mer, and one
    without any, among them)"""
    nks = [4000, 1, 0, 513, 5000, 16384 - 9514, 1, 0, 9000, 32769 - 16385 - 9000]
    assert sum(nks[:6]) == 16384 and sum(nks[:7]) == 16385 and sum(nks) == 32769
    seqs = reads_of_nk(np.random.default_rng(7800), nks)
    return oracle.concat(seqs)


@pytest.mark.parametrize("n_reads,total", [(6, 16384), (7, 16385), (10, 32769)])
@pytest.mark.parametrize("m", [257, 1110])
def test_all_seqs_chunks(ctx, oracle, all_seqs_batch, n_reads, total, m):
    """1, 2 and 3 chunks of super_chunk_count, reduced by k_super_reduce on 2 and 5 blocks"""
    bases, off = all_seqs_batch
    bases, off = bases[:int(off[n_reads])], off[:n_reads + 1]
    assert int((np.maximum(np.diff(off.astype(np.int64)) - K + 1, 0)).sum()) == total
    for form, hasher in (("f64", A.HASHER_NOHASH), ("u64", A.HASHER_FNV1A)):
        p = params(form, m, hasher, mode=A.MODE_ALL_SEQS)
        want = oracle.sketch(bases, off, p)
        assert want.shape == (1, m)
        same_bits(ctx.sketch(bases, off, p), want, "all seqs %d k-mers m %d %s" % (total, m, form))


def test_all_seqs_more_chunks_than_workgroups(ctx, oracle, n_cus):
    """pre-hashed values for three chunks more than the grid has workgroups at m = 1110 (one per CU): a workgroup that takes a
    second chunk starts it from the bound of an empty sketch"""
    n = 16384 * (n_cus + 2) + 1
    vals = np.random.default_rng(7850).integers(0, 2**63, n, dtype=np.uint64)
    off = np.array([0, n], np.uint64)
    for form in ("f64", "u64"):
        p = params(form, 1110, mode=A.MODE_ALL_SEQS, fhash=0)
        same_bits(ctx.sketch_hashed(vals, off, p), oracle.sketch_hashed(vals, off, p), "%d values %s" % (n, form))


def test_partials_of_three_shares(ctx, oracle, all_seqs_batch):
    """three shares of the reads sketched into partial slot minima and merged: the all-sequences row of the whole batch"""
    bases, off = all_seqs_batch
    for form in ("f64", "u32"):
        p = params(form, 588, A.HASHER_FNV1A, mode=A.MODE_ALL_SEQS)
        want = oracle.sketch(bases, off, p)
        parts = []
        for lo, hi in ((0, 3), (3, 7), (7, 10)):
            b = np.ascontiguousarray(bases[int(off[lo]):int(off[hi])])
            parts.append(ctx.sketch_partial(b, np.ascontiguousarray(off[lo:hi + 1] - off[lo]), p))
        got = ctx.sketch_merge_partials(np.ascontiguousarray(np.stack(parts)), p)
        same_bits(got.reshape(1, -1), want, "partials %s" % form)


# ---- i. one context, changing plans -----------------------------------------------------------------------------------------
def test_one_context_changing_plans(oracle, n_cus):
    """m = 1110 (one wave, 63 lanes, the attribute call, more reads than workgroups), then 64, then 226 (just over 64 KiB), then 1110
    again on a context of its own: the queue word, the output buffer and a grid that shrinks are reused from call to call"""
    from kmerutils_amd import lib
    big = _short_reads(oracle, 7900, n_cus + 9)
    mid = oracle.concat(reads_of_nk(np.random.default_rng(7901), [0, 1, 70, 300, 513] * 8))
    few = oracle.concat(reads_of_nk(np.random.default_rng(7902), [255, 0, 600]))
    c = lib.Context(0)
    try:
        rows = []
        for (bases, off), form, m in ((big, "u64", 1110), (mid, "f32", 64), (few, "f64", 226), (big, "u64", 1110)):
            p = params(form, m)
            got = np.array(c.sketch(bases, off, p))
            same_bits(got, oracle.sketch(bases, off, p), "m %d %s" % (m, form))
            rows.append(got)
        assert rows[0].tobytes() == rows[3].tobytes()
    finally:
        c.close()

"""The count prefilter on the device (kmu_kfilter_*, kmu_count_add_reads_filtered) against the numpy model of
tests/kfilter_model.py, which adds the occurrences one after the other, and against the oracle's counter.  The planes are a function
of the multiset of occurrences, so every comparison is for equality, word for word.

Reads: 120 reads of 300 bases of a 20 kb genome with 1 % substitutions; a poly-A read of 2 500 bases (one key, thousands of
simultaneous adds inside single waves); reads of k - 1, k and k + 1 bases; a read that ends exactly on a 1 024-base wave step,
then a short one.  Filter shapes: one cell with one hash and eight cells with eight hashes (crowded: plane B is far from trivial and
nearly every singleton passes), 1 000 cells, and the useful one, 16 bits per occurrence."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfilter_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

KMERS = [(A.KMER64BIT, 31), (A.KMER16B32BIT, 16)]
KMER_IDS = ["k31", "k16"]
SHAPES = [(1, 1), (8, 8), (1000, 4), (None, 4)]  # None: cells_for(occurrences, 16)
SHAPE_IDS = ["1x1", "8x8", "1000x4", "16bits"]


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def _cat(parts):
    bases = np.concatenate([b for b, _ in parts])
    lens = np.concatenate([np.diff(o.astype(np.int64)) for _, o in parts])
    off = np.zeros(lens.size + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    return bases, off


def added_reads(k):
    b, o = synth.genome_reads(120, np.full(120, 300, np.int64), 20_000, 0xA1, sub=0.01)
    poly = np.frombuffer(b"A" * 2500, np.uint8)
    lens = [k - 1, k, k + 1]
    tot = 120 * 300 + 2500 + sum(lens)
    lens += [300 + (-(tot + 300)) % 1024, 35]  # a read that ends exactly on a step boundary, then a short one
    assert (tot + lens[-2]) % 1024 == 0
    tail = synth.genome_reads(len(lens), np.array(lens, np.int64), 20_000, 0xA1, sub=0.01)
    return _cat([(b, o), (poly, np.array([0, 2500], np.uint64)), tail])


def occurrences(oracle, bases, off, ktype, k):
    """the canonical k-mer of every k-mer start, in (sequence, position) order"""
    canon = oracle.kmer_hashes(bases, off, ktype, k, A.FHASH_CANON_VALUE)
    keep = np.zeros(canon.size, bool)
    for i in range(off.size - 1):
        keep[int(off[i]):int(off[i]) + max(int(off[i + 1]) - int(off[i]) - k + 1, 0)] = True
    return canon[keep].astype(np.uint64)


_CASES = {}


def case(oracle, ktype, k):
    """computed once per k-mer type, shared, never changed"""
    if (ktype, k) not in _CASES:
        b, o = added_reads(k)
        occ = occurrences(oracle, b, o, ktype, k)
        oc = oracle.Counter(ktype, k, 16, 1 << 20)
        oc.add_reads(b, o)
        ob, oo = synth.genome_reads(40, np.full(40, 300, np.int64), 20_000, 0xB2)  # another genome: k-mers never added
        _CASES[(ktype, k)] = {"bases": b, "off": o, "occ": occ, "oracle": oc, "dump1": oc.dump(1),
                              "other": occurrences(oracle, ob, oo, ktype, k), "planes": {}}
    return _CASES[(ktype, k)]


def shape_of(cs, shape):
    n_cells, n_hashes = shape
    return (M.cells_for(cs["occ"].size, 16) if n_cells is None else n_cells), n_hashes


def planes_of(cs, n_cells, n_hashes):
    if (n_cells, n_hashes) not in cs["planes"]:
        cs["planes"][(n_cells, n_hashes)] = M.build(cs["occ"], n_cells, n_hashes)
    return cs["planes"][(n_cells, n_hashes)]


def dev(x):
    import torch
    return torch.from_numpy(x.astype(np.int64) if x.dtype == np.uint64 else x).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_planes_and_info(ctx, oracle, ktype, k, shape):
    import torch
    cs = case(oracle, ktype, k)
    n_cells, n_hashes = shape_of(cs, shape)
    b, o, occ = cs["bases"], cs["off"], cs["occ"]
    planes = planes_of(cs, n_cells, n_hashes)
    want = M.words(planes)
    assert (planes[1] != 0).any()  # (plane B is in play at every shape)
    f = ctx.kfilter(ktype, k, n_cells, n_hashes)
    assert not f.export().any() and f.info()["n_added"] == 0
    # one call; host memory
    f.add_reads(b, o)
    assert np.array_equal(f.export(), want)
    assert np.array_equal(host(f.export(device=torch.device("cuda", 0))), want)
    info = f.info()
    bits_a, bits_b = M.popcount(planes[0]), M.popcount(planes[1])
    assert (info["n_cells"], info["bytes"], info["n_hashes"], info["kmer_size"]) == (n_cells, 16 * n_cells, n_hashes, k)
    assert (info["n_added"], info["bits_a"], info["bits_b"]) == (occ.size, bits_a, bits_b)
    est = M.est_distinct(n_cells, n_hashes, bits_a)
    if math.isinf(est):
        assert math.isinf(info["est_distinct"]) and info["est_distinct"] > 0
    else:
        assert abs(info["est_distinct"] - est) <= 1e-12 * est
    # the same reads in three calls, in reversed order (ranges of the read set: offsets[0] != 0), from device memory
    f.reset()
    assert not f.export().any()
    n = o.size - 1
    db, do = dev(b), dev(o)
    for first, last in ((122, n), (60, 122), (0, 60)):
        f.add_reads(db, do[first:last + 1])
    assert np.array_equal(f.export(), want) and f.info()["n_added"] == occ.size
    # ... and from host memory
    f.reset()
    for first, last in ((122, n), (60, 122), (0, 60)):
        f.add_reads(b, o[first:last + 1])
    assert np.array_equal(f.export(), want)
    # the canonical values themselves, host and device
    f.reset()
    f.add_kmers(occ[:1000])
    f.add_kmers(dev(occ[1000:]))
    assert np.array_equal(f.export(), want) and f.info()["n_added"] == occ.size
    f.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_query(ctx, oracle, ktype, k, shape):
    cs = case(oracle, ktype, k)
    n_cells, n_hashes = shape_of(cs, shape)
    planes = planes_of(cs, n_cells, n_hashes)
    f = ctx.kfilter(ktype, k, n_cells, n_hashes)
    f.add_reads(cs["bases"], cs["off"])
    keys = np.concatenate([cs["occ"], cs["other"]])
    want = M.classes(planes, keys, n_hashes)
    got = f.query(keys)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(f.query(dev(keys)).cpu().numpy(), want)
    uk, uc = cs["dump1"]
    assert (M.classes(planes, uk[uc >= 2], n_hashes) == 2).all() and (want[:cs["occ"].size] >= 1).all()
    if shape[0] is None:  # the useful shape tells things apart
        assert (want[cs["occ"].size:] == 0).mean() > 0.9 and (M.classes(planes, uk[uc == 1], n_hashes) == 1).mean() > 0.9
    assert f.query(np.zeros(0, np.uint64)).size == 0
    f.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_merge(ctx, oracle, ktype, k, shape):
    from kmerutils_amd import lib
    cs = case(oracle, ktype, k)
    n_cells, n_hashes = shape_of(cs, shape)
    b, o = cs["bases"], cs["off"]
    want = M.words(planes_of(cs, n_cells, n_hashes))
    n = o.size - 1
    f1, f2 = ctx.kfilter(ktype, k, n_cells, n_hashes), ctx.kfilter(ktype, k, n_cells, n_hashes)
    f1.add_reads(b, o[:61])
    f2.add_reads(b, o[60:n + 1])
    half = f1.export()
    f1.merge(f2)
    assert np.array_equal(f1.export(), want) and f1.info()["n_added"] == cs["occ"].size
    # the model's merge says the same
    p1 = (half[0::2], half[1::2])
    w2 = f2.export()
    assert np.array_equal(M.words(M.merge(p1, (w2[0::2], w2[1::2]))), want)
    # other parameters: refused, dst as it was
    others = [ctx.kfilter(ktype, k, n_cells + 1, n_hashes), ctx.kfilter(ktype, k, n_cells, n_hashes % 8 + 1)]
    if ktype == A.KMER64BIT:
        others += [ctx.kfilter(ktype, k - 1, n_cells, n_hashes)]
    for other in others:
        other.add_reads(b, o[:10])
        with pytest.raises(lib.KmuError) as e:
            f1.merge(other)
        assert e.value.code == A.E_BAD_ARG
        other.close()
    assert np.array_equal(f1.export(), want) and f1.info()["n_added"] == cs["occ"].size
    f1.close()
    f2.close()


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_select_reads(ctx, oracle, ktype, k, shape):
    import torch
    cs = case(oracle, ktype, k)
    n_cells, n_hashes = shape_of(cs, shape)
    b, o, occ = cs["bases"], cs["off"], cs["occ"]
    planes = planes_of(cs, n_cells, n_hashes)
    want = occ[M.classes(planes, occ, n_hashes) == 2]
    f = ctx.kfilter(ktype, k, n_cells, n_hashes)
    f.add_reads(b, o)
    assert f.n_passing(b, o) == want.size  # the size query
    got = f.select_reads(b, o)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    db, do = dev(b), dev(o)
    assert np.array_equal(host(f.select_reads(db, do)), want)
    # `offsets + first` of device-resident reads
    nk = np.maximum(np.diff(o.astype(np.int64)) - k + 1, 0)
    start = np.concatenate([[0], np.cumsum(nk)])
    for first, last in ((5, 30), (119, o.size - 1), (121, 124)):
        sub = occ[start[first]:start[last]]
        wsub = sub[M.classes(planes, sub, n_hashes) == 2]
        assert np.array_equal(host(f.select_reads(db, do[first:last + 1])), wsub), (first, last)
        assert np.array_equal(f.select_reads(b, o[first:last + 1]), wsub), (first, last)
    # cap one short: refused, the total reported, the output untouched
    L = ctx.L
    vp = C.c_void_p
    out = np.full(want.size + 4, 0x5A5A, np.uint64)
    n = C.c_uint64(0)
    rc = L.kmu_kfilter_select_reads(f.h, b.ctypes.data_as(vp), o.ctypes.data_as(vp), o.size - 1, A.MEM_HOST, out.ctypes.data_as(vp),
                                    want.size - 1, C.byref(n))
    assert rc == A.E_BAD_ARG and n.value == want.size and (out == 0x5A5A).all()
    dout = torch.full((want.size + 4,), 0x5A5A, dtype=torch.int64, device="cuda")
    rc = L.kmu_kfilter_select_reads(f.h, vp(db.data_ptr()), vp(do.data_ptr()), o.size - 1, A.MEM_DEVICE, vp(dout.data_ptr()), want.size - 1,
                                    C.byref(n))
    assert rc == A.E_BAD_ARG and n.value == want.size and bool((dout == 0x5A5A).all())
    # no sequence at all; nothing but sequences shorter than k
    assert f.select_reads(b[:16], np.array([0], np.uint64)).size == 0
    assert f.select_reads(b[:40], np.array([0, 0, 10, 10 + k - 1], np.uint64)).size == 0
    f.close()


@pytest.mark.parametrize("chunk", [None, "4096"], ids=["onechunk", "chunk4096"])
@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("ktype,k", KMERS, ids=KMER_IDS)
def test_add_reads_filtered(ctx, oracle, monkeypatch, ktype, k, shape, path, chunk):
    from kmerutils_amd import lib
    monkeypatch.setenv("KMU_COUNT_PATH", path)
    if chunk:
        monkeypatch.setenv("KMU_KFILTER_CHUNK_KMERS", chunk)
    cs = case(oracle, ktype, k)
    n_cells, n_hashes = shape_of(cs, shape)
    b, o, occ = cs["bases"], cs["off"], cs["occ"]
    planes = planes_of(cs, n_cells, n_hashes)
    uk, uc = cs["dump1"]  # every distinct k-mer with its true count, sorted by k-mer
    passing = M.classes(planes, uk, n_hashes) == 2
    assert passing[uc >= 2].all()  # every k-mer seen at least twice is among those that pass
    n_pass = int((M.classes(planes, occ, n_hashes) == 2).sum())
    assert n_pass == int(uc[passing].sum())
    if chunk:
        assert n_pass > 2 * int(chunk)  # several chunks
    f = ctx.kfilter(ktype, k, n_cells, n_hashes)
    f.add_reads(b, o)
    plain = ctx.counter(ktype, k, 8, 1 << 16)
    plain.add_reads(b, o)
    for bb, oo in ((b, o), (dev(b), dev(o))):
        c = ctx.counter(ktype, k, 8, 1 << 16)
        before = c.nb_occurrences()
        got_pass = c.add_reads_filtered(f, bb, oo)
        assert got_pass == n_pass and c.nb_occurrences() - before == got_pass
        gk, gc = c.dump(1)
        assert np.array_equal(gk, uk[passing]) and np.array_equal(gc, np.minimum(uc[passing], 255))
        assert gc.max() == 255  # (the poly-A k-mer: saturated)
        pk, pc = plain.dump(2)
        g2k, g2c = c.dump(2)
        assert np.array_equal(g2k, pk) and np.array_equal(g2c, pc)
        assert c.nb_unique() == int((uc[passing] == 1).sum())  # the singletons that slipped through
        c.close()
    # a non-ACGT byte: refused before anything is added
    bad = b.copy()
    bad[777] = ord("N")
    c = ctx.counter(ktype, k, 8, 1 << 16)
    with pytest.raises(lib.KmuError) as e:
        c.add_reads_filtered(f, bad, o)
    assert e.value.code == A.E_NON_ACGT and e.value.n_passed == 0 and c.nb_distinct() == 0
    with pytest.raises(lib.KmuError) as e:
        f.add_reads(bad, o)
    assert e.value.code == A.E_NON_ACGT
    c.close()
    plain.close()
    f.close()


def test_refusals(ctx, oracle):
    from kmerutils_amd import lib
    cs = case(oracle, A.KMER64BIT, 31)
    b, o = cs["bases"], cs["off"]
    for kw in ({"n_hashes": 0}, {"n_hashes": 9}, {"n_cells": 0}, {"n_cells": 1 << 32}, {"kmer_type": A.KMERAA64BIT, "k": 8}, {"k": 33}):
        args = {"kmer_type": A.KMER64BIT, "k": 31, "n_cells": 100, "n_hashes": 4}
        args.update(kw)
        with pytest.raises(lib.KmuError) as e:
            ctx.kfilter(**args)
        assert e.value.code in (A.E_BAD_ARG, A.E_BAD_K, A.E_BAD_ALPHABET), kw
        if "n_hashes" in kw or "n_cells" in kw:
            assert e.value.code == A.E_BAD_ARG
    f = ctx.kfilter(A.KMER64BIT, 31, 100, 4)
    f.add_reads(b, o)
    # a counter of another size, of another type, of another context
    other = lib.Context(0)
    for c in (ctx.counter(A.KMER64BIT, 30, 8, 1 << 16), ctx.counter(A.KMER16B32BIT, 16, 8, 1 << 16), other.counter(A.KMER64BIT, 31, 8, 1 << 16)):
        with pytest.raises(lib.KmuError) as e:
            c.add_reads_filtered(f, b, o)
        assert e.value.code == A.E_BAD_ARG and c.nb_distinct() == 0
        c.close()
    other.close()
    # no sequence at all
    c = ctx.counter(A.KMER64BIT, 31, 8, 1 << 16)
    assert c.add_reads_filtered(f, b[:16], np.array([0], np.uint64)) == 0 and c.nb_distinct() == 0
    c.close()
    f.close()


def test_distributed_counter_is_unsupported(oracle, monkeypatch):
    from kmerutils_amd import lib
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", os.environ.get("NCCL_SOCKET_IFNAME", "lo"))
    cs = case(oracle, A.KMER64BIT, 31)
    ctx = lib.Context(0)
    ctx.comm_init(lib.Context.comm_get_id(), 0, 1)
    c = ctx.counter(A.KMER64BIT, 31, 8, 1 << 16, distributed=True)
    f = ctx.kfilter(A.KMER64BIT, 31, 100, 4)
    with pytest.raises(lib.KmuError) as e:
        c.add_reads_filtered(f, cs["bases"], cs["off"])
    assert e.value.code == A.E_UNSUPPORTED
    f.close()
    c.close()
    ctx.comm_destroy()
    ctx.close()


def test_mirror_and_tool(ctx, oracle, tmp_path):
    """count_repeated_kmers, and `parsefastq --count --repeated`: the dump is byte for byte that of the plain count"""
    from kmerutils_amd import kmercount, parsefastq
    cs = case(oracle, A.KMER64BIT, 31)
    b, o, occ = cs["bases"], cs["off"], cs["occ"]
    uk, uc = cs["dump1"]
    kc, kf = kmercount.count_repeated_kmers((b, o), 31, 8, ctx=ctx)
    n_cells = M.cells_for(occ.size, 16)
    planes = planes_of(cs, n_cells, 4)
    assert np.array_equal(kf.words(), M.words(planes)) and kf.info()["n_added"] == occ.size
    assert np.array_equal(kf.seen_class(uk), M.classes(planes, uk, 4))
    ak, ac = kc.above2_entries()
    assert np.array_equal(ak, uk[uc >= 2]) and np.array_equal(ac, np.minimum(uc[uc >= 2], 255))
    assert np.array_equal(kc.get_above2_count(uk), np.where(uc >= 2, np.minimum(uc, 255), 0))
    passing = M.classes(planes, uk, 4) == 2
    assert kc.get_nb_distinct() == int(passing.sum()) < uk.size // 2 and kc.get_nb_unique() == int((uc[passing] == 1).sum())
    single = kmercount.KmerPrefilter(31, n_cells, ctx=ctx)
    single.insert_kmer(int(uk[0]))
    single.insert_kmer(uk[1:3])
    single.insert_kmer(uk[1:2])
    assert single.seen_class(uk[:4]).tolist() == [1, 2, 1, 0]
    other = kmercount.KmerPrefilter(31, n_cells, ctx=ctx)
    other.insert_kmer(uk[0:1])
    single.merge(other)
    assert single.seen_class(uk[:4]).tolist() == [2, 2, 1, 0]
    # the tool
    fq = tmp_path / "tiny.fastq"
    with open(fq, "w") as fh:
        for i in list(range(40)) + [120]:
            s = b[int(o[i]):int(o[i + 1])].tobytes().decode()
            fh.write("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    plain_dir, rep_dir = tmp_path / "plain", tmp_path / "rep"
    plain_dir.mkdir()
    rep_dir.mkdir()
    assert parsefastq.main(["-f", str(fq), "-s", "31", "--outdir", str(plain_dir)]) == 0
    assert parsefastq.main(["-f", str(fq), "-s", "31", "--outdir", str(rep_dir), "--repeated", "--filter-bits", "12"]) == 0
    want = (plain_dir / "tiny.fastq.multi_kmer.bin").read_bytes()
    assert len(want) > 1000 and (rep_dir / "tiny.fastq.multi_kmer.bin").read_bytes() == want
    with pytest.raises(SystemExit):
        parsefastq.main(["-f", str(fq), "-s", "31", "--outdir", str(rep_dir), "--repeated", "--histo", str(tmp_path / "h")])
    # the C++ tool: its two dumps are the same file too
    from kmerutils_amd import build
    import subprocess
    exe = [p for p in build.build_host() if p.endswith("parsefastq")][0]
    dumps = []
    for name, extra in (("cpp_plain", []), ("cpp_rep", ["--repeated"])):
        (tmp_path / name).mkdir()
        r = subprocess.run([exe, "-f", str(fq), "kmer", "--count", "-s", "31", "--outdir", str(tmp_path / name)] + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        dumps.append((tmp_path / name / "tiny.fastq.multi_kmer.bin").read_bytes())
    assert len(dumps[0]) > 1000 and dumps[0] == dumps[1]
    r = subprocess.run([exe, "-f", str(fq), "kmer", "--count", "-s", "31", "--repeated", "--histo", str(tmp_path / "h")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "meaningless" in r.stderr

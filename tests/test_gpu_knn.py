"""GPU: kmu_sig_knn (exact k nearest neighbours of signature rows) against a numpy restatement of its contract, through
the binding, the Python helpers and both datasketcher front ends.  Every comparison is integer and exact."""
import os
import subprocess

import numpy as np
import pytest

from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context(0)
    yield c
    c.close()


def knn_ref(q, db, k, gq=None, gdb=None):
    eq = (q[:, None, :] == db[None, :, :]).sum(-1).astype(np.int64)
    ok = np.ones(eq.shape, bool) if gq is None else gq[:, None] != gdb[None, :]
    idx = np.full((len(q), k), 0xFFFFFFFF, np.uint32); cnt = np.zeros((len(q), k), np.uint16)
    for i in range(len(q)):
        j = np.flatnonzero(ok[i])
        o = j[np.lexsort((j, -eq[i, j]))][:k]          # eq descending, index ascending
        idx[i, :len(o)] = o; cnt[i, :len(o)] = eq[i, o]
    return idx, cnt


def graded(seed, nq, ndb, m, dtype=np.uint32):
    """database rows over an alphabet of 4 values, queries = copies of database rows with a per-row random fraction of
    slots changed: graded similarity, ties inside the lists"""
    rng = np.random.default_rng(seed)
    db = rng.integers(0, 4, size=(ndb, m)).astype(np.uint64)
    src = rng.integers(0, ndb, size=nq)
    q = db[src].copy()
    frac = rng.random(nq)
    change = rng.random((nq, m)) < frac[:, None]
    q[change] = rng.integers(0, 4, size=int(change.sum())).astype(np.uint64)
    if np.dtype(dtype).kind == "f":   # raw words: distinct small integers are distinct floats, compared bit for bit
        return q.astype(dtype), db.astype(dtype)
    if np.dtype(dtype).itemsize == 8:  # values that differ in the upper word only, too
        q, db = q << np.uint64(31), db << np.uint64(31)
    return q.astype(dtype), db.astype(dtype)


def raw(a):
    return a.view(np.uint32 if a.itemsize == 4 else np.uint64)


def check(ctx, q, db, k, gq=None, gdb=None):
    idx, eq = ctx.sig_knn(q, db, k, gq, gdb)
    widx, weq = knn_ref(raw(q), raw(db), k, gq, gdb)
    assert idx.dtype == np.uint32 and eq.dtype == np.uint16 and idx.shape == (len(q), k)
    assert np.array_equal(idx, widx) and np.array_equal(eq, weq)
    return idx, eq


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64, np.float32, np.float64])
@pytest.mark.parametrize("m", [7, 33, 64, 200])
def test_types_and_sketch_sizes(ctx, dtype, m):
    for nq, ndb, k in ((130, 1000, 10), (1, 1, 1), (65, 63, 64), (65, 63, 1)):
        q, db = graded(1000 * m + nq, nq, ndb, m, dtype)
        check(ctx, q, db, k)


def test_graded_inputs_are_graded(ctx):
    q, db = graded(7, 130, 1000, 200)
    idx, eq = check(ctx, q, db, 10)
    assert len(np.unique(eq)) > 50 and all(len(np.unique(r)) < 10 for r in eq)  # many levels, and a tie in every list


def test_k_above_ndb_and_empty_database(ctx):
    q, db = graded(3, 70, 9, 33)
    idx, eq = check(ctx, q, db, 64)
    assert (idx[:, 9:] == NONE).all() and (eq[:, 9:] == 0).all() and (np.sort(idx[:, :9], 1) == np.arange(9)).all()
    idx, eq = ctx.sig_knn(q, db[:0], 5)
    assert idx.shape == (70, 5) and (idx == NONE).all() and (eq == 0).all()
    idx, eq = ctx.sig_knn(q[:0], db, 5)
    assert idx.shape == (0, 5) and eq.shape == (0, 5)


def test_ties_only(ctx):
    same = np.tile(np.arange(20, dtype=np.uint32), (300, 1))
    idx, eq = check(ctx, same[:70], same, 12)
    assert (idx == np.arange(12)).all() and (eq == 20).all()
    q = np.zeros((70, 20), np.uint32)
    db = np.arange(1, 300 * 20 + 1, dtype=np.uint32).reshape(300, 20)   # eq = 0 everywhere
    idx, eq = check(ctx, q, db, 12)
    assert (idx == np.arange(12)).all() and (eq == 0).all()
    g = np.arange(70, dtype=np.uint32)
    idx, eq = check(ctx, q, db, 12, g, np.arange(300, dtype=np.uint32))
    assert all(idx[i].tolist() == [j for j in range(13) if j != i][:12] for i in range(70))


def test_groups(ctx):
    _, db = graded(11, 1, 500, 33)
    db[100] = db[7]; db[333] = db[7]                     # identical duplicate rows
    g = np.arange(500, dtype=np.uint32)
    idx, eq = check(ctx, db, db, 10, g, g)               # self-join
    assert not (idx == g[:, None]).any()
    assert idx[7, :2].tolist() == [100, 333] and idx[100, :2].tolist() == [7, 333] and (eq[7, :2] == 33).all()
    g3 = g // 3                                          # block-like groups
    idx, eq = check(ctx, db, db, 10, g3, g3)
    assert not (g3[idx] == g3[:, None]).any()
    gq = np.array([5, 9], np.uint32)                     # a query whose group covers the whole database
    idx, eq = check(ctx, db[:2], db, 10, gq, np.full(500, 5, np.uint32))
    assert (idx[0] == NONE).all() and (eq[0] == 0).all() and (idx[1] != NONE).all()


def test_segments_and_slabs(monkeypatch):
    from kmerutils_amd import lib
    q, db = graded(21, 100, 20000, 16)
    gq = np.arange(100, dtype=np.uint32)
    gdb = np.arange(20000, dtype=np.uint32)
    want = knn_ref(q, db, 10, gq, gdb)
    got = {}
    for name, env in (("default", {}), ("segments", {"KMU_KNN_SEG_ROWS": "300"}),
                      ("segments+slabs", {"KMU_KNN_SEG_ROWS": "128", "KMU_KNN_WS_MB": "1"})):
        for k_, v in env.items():
            monkeypatch.setenv(k_, v)
        c = lib.Context(0)
        c.profile_enable(True)
        got[name] = c.sig_knn(q, db, 10, gq, gdb)
        prof = c.profile_get()
        c.close()
        assert prof["k_sig_knn"][0] == prof["k_sig_knn_merge"][0] == (2 if name == "segments+slabs" else 1), prof
    for name, (idx, eq) in got.items():
        assert np.array_equal(idx, want[0]) and np.array_equal(eq, want[1]), name


def test_device_tensors(ctx):
    import torch
    for dtype, tdt in ((np.uint32, np.int32), (np.uint64, np.int64)):
        q, db = graded(31, 130, 777, 64, dtype)
        gq = np.arange(130, dtype=np.uint32) % 50
        gdb = np.arange(777, dtype=np.uint32) % 50
        hidx, heq = check(ctx, q, db, 10, gq, gdb)
        tq, tdb = torch.from_numpy(q.view(tdt)).cuda(), torch.from_numpy(db.view(tdt)).cuda()
        didx, deq = ctx.sig_knn(tq, tdb, 10, torch.from_numpy(gq.view(np.int32)).cuda(), torch.from_numpy(gdb.view(np.int32)).cuda())
        ctx.synchronize()
        assert didx.is_cuda and deq.is_cuda
        assert np.array_equal(didx.cpu().numpy().view(np.uint32), hidx) and np.array_equal(deq.cpu().numpy().view(np.uint16), heq)
    mat = ctx.sig_equal_matrix(q, db)
    assert np.array_equal(heq, np.take_along_axis(mat, hidx.astype(np.int64), 1))


def _mutated_reads():
    from kmerutils_amd import synth
    bases, off = synth.uniform_reads(300, 2000, 0xAB)
    rng = np.random.default_rng(5)
    reads = [bases[int(off[i]):int(off[i + 1])] for i in range(300)]
    origin = rng.choice(300, size=60, replace=False)
    for o in origin:   # copies with 2 % of the bases substituted
        r = reads[o].copy()
        pos = np.flatnonzero(rng.random(len(r)) < 0.02)
        r[pos] = synth.ACGT[(np.searchsorted(synth.ACGT, r[pos]) + rng.integers(1, 4, size=len(pos))) % 4]
        reads.append(r)
    return [bytes(r) for r in reads], origin


def test_real_signatures(ctx, oracle):
    """ProbMinHash3a signatures (k = 8, m = 200, datasketcher's parameters) of synthetic reads plus mutated copies"""
    from kmerutils_amd import sketching as S
    reads, origin = _mutated_reads()
    p = A.SketchParams(A.ALGO_PROB3A, A.KMER32BIT, 8, 200, A.SIG_U32, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH, 0, 0, 0, 0, 0)
    bases, off = oracle.concat(reads)
    want_sig = oracle.sketch(bases, off, p)
    g = np.arange(len(reads), dtype=np.uint32)
    widx, weq = knn_ref(want_sig, want_sig, 5, g, g)
    assert np.array_equal(widx[300:, 0], origin), "the mutation rate does not plant every pair: lower it"  # CPU, oracle
    sig = np.asarray(S.SeqSketcher(8, 200, ctx=ctx).sketch_probminhash3a(reads, A.FHASH_CANON_INVHASH))
    idx, eq = ctx.sig_knn(sig, sig, 5, g, g)
    assert np.array_equal(idx, widx) and np.array_equal(eq, weq)
    assert np.array_equal(idx[300:, 0], origin)
    nidx, dist = S.nearest_neighbours(sig, sig, 5, g, g, ctx=ctx)
    assert np.array_equal(nidx, widx) and dist.dtype == np.float32
    assert np.array_equal(dist, (np.float32(200) - weq.astype(np.float32)) / np.float32(200))
    nidx, dist = S.nearest_neighbours(sig[:3], sig[:2], 4, ctx=ctx)
    assert (nidx[:, 2:] == NONE).all() and (dist[:, 2:] == 1.0).all()


def test_block_nearest_neighbours(ctx):
    from kmerutils_amd import sketching as S
    reads, _ = _mutated_reads()
    rows, numseq, _ = S.BlockSeqSketcher(500, 8, 64, ctx=ctx).blocksketch_sequences(reads[:40], A.FHASH_CANON_INVHASH)
    rows = np.asarray(rows)
    idx, dist = S.block_nearest_neighbours(rows, numseq, 6, ctx=ctx)
    widx, weq = knn_ref(rows, rows, 6, numseq, numseq)
    assert np.array_equal(idx, widx) and not (numseq[idx] == numseq[:, None]).any()
    assert np.array_equal(dist, (np.float32(64) - weq.astype(np.float32)) / np.float32(64))


def test_errors(ctx):
    from kmerutils_amd.lib import KmuError
    q, db = graded(1, 10, 20, 16)
    g = np.arange(20, dtype=np.uint32)
    for args, code in (((q, db, 0), A.E_BAD_ARG), ((q, db, 65), A.E_UNSUPPORTED), ((q[:, :0], db[:, :0], 3), A.E_BAD_ARG),
                       ((q, db, 3, g[:10], None), A.E_BAD_ARG), ((q, db, 3, None, g), A.E_BAD_ARG)):
        with pytest.raises(KmuError) as e:
            ctx.sig_knn(*args)
        assert e.value.code == code
    check(ctx, q, db, 3)   # the context still works


def _fastq(tmp_path):
    reads, _ = _mutated_reads()
    fn = tmp_path / "reads.fastq"
    fn.write_bytes(b"".join(b"@r%d\n" % i + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in enumerate(reads[250:])))
    return str(fn)


@pytest.mark.parametrize("block", [0, 700])
def test_tools_ann(tmp_path, block):
    from kmerutils_amd import build as kbuild
    from kmerutils_amd import datasketcher, formats
    kbuild.build_host()
    exe = os.path.join(ROOT, "kmerutils_amd", "bin", "datasketcher")
    fq = _fastq(tmp_path)
    common = ["-f", fq, "-k", "8", "-s", "64"] + (["-b", str(block)] if block else [])
    py, cpp, plain = str(tmp_path / "py.sig"), str(tmp_path / "cpp.sig"), str(tmp_path / "plain.sig")
    assert datasketcher.main(common + ["-d", py, "ann", "--nb", "5"]) == 0
    r = subprocess.run([exe] + common + ["-d", cpp, "ann", "--nb", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert datasketcher.main(common + ["-d", plain]) == 0
    assert not os.path.exists(plain + "-ann")
    assert open(py, "rb").read() == open(plain, "rb").read() == open(cpp, "rb").read()
    assert open(py + "-ann", "rb").read() == open(cpp + "-ann", "rb").read()
    if block:
        rd = formats.SigBlockSketchFileReader(py)
        rows, group = [], []
        while True:
            nxt = rd.next()
            if nxt is None:
                break
            rows += [b[1] for b in nxt[1]]
            group += [nxt[0]] * len(nxt[1])
        rows, group = np.array(rows), np.array(group, np.uint32)
        assert len(set(group)) < len(group)
    else:
        rows = formats.SigSketchFileReader(py).read_all()
        group = np.arange(len(rows), dtype=np.uint32)
    idx, eq, m = formats.read_neighbour_file(py + "-ann")
    widx, weq = knn_ref(rows, rows, 5, group, group)
    assert m == 64 and np.array_equal(idx, widx) and np.array_equal(eq, weq)

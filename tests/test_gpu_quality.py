"""The quality line through the ingest (kmu_ingest_fastq_qual), the remap (kmu_quality_remap) and the per-read class statistics
(kmu_read_qual_stats) on the device, exact equality against tests/read_stats_model.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_stats_model as M  # noqa: E402

pytestmark = pytest.mark.gpu
QUAL = np.dtype(A.READ_QUAL_DTYPE)


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context()
    yield c
    c.close()


def records(n=40, seed=5):
    """(sequence, quality, line end) per record: lengths 0 .. 2100, "\\r\\n" on some, records with N between kept ones"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        length = [0, 1, 16, 17, 1024, 1025, 2100][i % 7] if i % 3 == 0 else int(rng.integers(1, 300))
        seq = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), length)
        if i % 6 == 4 and length:
            seq[int(rng.integers(0, length))] = ord("N")
        qual = rng.integers(0x21, 0x7F, length).astype(np.uint8)
        out.append((seq.tobytes(), qual.tobytes(), b"\r\n" if i % 4 == 1 else b"\n"))
    return out


def fastq(recs, final_newline=False):
    text = b"".join(b"@read%d" % i + e + s + e + b"+" + e + q + e for i, (s, q, e) in enumerate(recs))
    last = recs[-1][2]
    return text if final_newline else text[:-len(last)]


def device_text(text):
    import torch
    pad = np.zeros(len(text) + 64, np.uint8)
    pad[:len(text)] = np.frombuffer(text, np.uint8)
    return torch.from_numpy(pad).cuda()[:len(text)]


def info_tuple(info):
    return tuple(int(getattr(info, name)) for name, _ in A.IngestInfo._fields_)


@pytest.mark.parametrize("final_newline", [False, True], ids=["no_final_newline", "final_newline"])
def test_ingest_with_qualities_is_the_ingest_plus_the_quality_lines(ctx, final_newline):
    recs = records()
    assert recs[-1][2] == b"\n" and sum(1 for s, _, _ in recs if b"N" in s) >= 4
    text = fastq(recs, final_newline)
    want = M.ingest_fastq_qual(text)
    b0, o0, i0, x0 = ctx.ingest_fastq(text, want_index=True)
    bases, quals, off, info, idx = ctx.ingest_fastq_qual(text, want_index=True)
    assert np.array_equal(bases, b0) and np.array_equal(off, o0) and np.array_equal(idx, x0) and info_tuple(info) == info_tuple(i0)
    assert np.array_equal(bases, want[0]) and np.array_equal(quals, want[1]) and np.array_equal(off, want[2]) and np.array_equal(idx, want[3])
    assert info.n_records == 40 and info.n_kept == want[3].size < 40  # none of a dropped record's qualities appear
    # the same text on the device
    d = ctx.ingest_fastq_qual(device_text(text), want_index=True)
    assert np.array_equal(d[0].cpu().numpy(), want[0]) and np.array_equal(d[1].cpu().numpy(), want[1])
    assert np.array_equal(d[2].cpu().numpy().view(np.uint64), want[2]) and np.array_equal(d[4].cpu().numpy().view(np.uint32), want[3])
    assert info_tuple(d[3]) == info_tuple(i0)


def test_the_text_may_end_in_a_carriage_return(ctx):
    """a last record in "\\r\\n" form whose final newline is missing: the "\\r" that ends the text is no quality byte"""
    text = b"@a\r\nACGTAC\r\n+\r\nIIII%%\r\n@b\r\nGGTT\r\n+\r\n7777\r"
    want = M.ingest_fastq_qual(text)
    bases, quals, off, info = ctx.ingest_fastq_qual(text)
    assert quals.tobytes() == b"IIII%%7777" and bases.tobytes() == b"ACGTACGGTT" and off.tolist() == [0, 6, 10]
    assert np.array_equal(quals, want[1]) and np.array_equal(off, want[2]) and info.n_kept == 2


def test_sizes_only_call(ctx):
    text = np.frombuffer(fastq(records()), np.uint8)
    a, b = A.IngestInfo(), A.IngestInfo()
    p = text.ctypes.data_as(C.c_void_p)
    ctx._check(ctx.L.kmu_ingest_fastq(ctx.h, p, text.size, A.MEM_HOST, None, 0, None, 0, None, C.byref(a)))
    ctx._check(ctx.L.kmu_ingest_fastq_qual(ctx.h, p, text.size, A.MEM_HOST, None, 0, None, 0, None, 0, None, C.byref(b)))
    assert info_tuple(a) == info_tuple(b) and b.n_records == 40 and b.kept_bases > 0


@pytest.mark.parametrize("which", ["kept", "dropped"])
def test_a_short_quality_line_is_an_invalid_record(ctx, which):
    from kmerutils_amd import lib
    recs = records()
    at = next(i for i, (s, _, _) in enumerate(recs) if len(s) > 20 and (b"N" in s) == (which == "dropped"))
    s, q, e = recs[at]
    recs[at] = (s, q[:-1], e)
    text = np.frombuffer(fastq(recs), np.uint8)
    bases, quals, offs = np.full(200_000, 7, np.uint8), np.full(200_000, 7, np.uint8), np.full(64, 7, np.uint64)
    info = A.IngestInfo()
    rc = ctx.L.kmu_ingest_fastq_qual(ctx.h, lib._ptr(text)[0], text.size, A.MEM_HOST, lib._ptr(bases)[0], bases.size, lib._ptr(quals)[0], quals.size,
                                     lib._ptr(offs)[0], offs.size, None, C.byref(info))
    assert rc == A.E_BAD_ARG and (bases == 7).all() and (quals == 7).all() and (offs == 7).all()
    with pytest.raises(lib.KmuError) as err:
        ctx.ingest_fastq_qual(text)
    assert err.value.code == A.E_BAD_ARG and "invalid record" in str(err.value)
    ctx.ingest_fastq(text)  # (the ingest without qualities does not look at the line)


def test_quality_remap_all_bytes(ctx):
    import torch
    q = np.tile(np.arange(256, dtype=np.uint8), 5)[:1237]  # (no multiple of 16)
    assert np.array_equal(ctx.quality_remap(q), M.QUAL_CLASS[q])
    for first in (0, 3):  # an aligned and an unaligned device array
        d = torch.from_numpy(q).cuda()[first:]
        assert np.array_equal(ctx.quality_remap(d).cpu().numpy(), M.QUAL_CLASS[q[first:]])
        assert np.array_equal(ctx.quality_remap(d, out=d).cpu().numpy(), M.QUAL_CLASS[q[first:]])  # in place
    h = q.copy()
    assert ctx.quality_remap(h, out=h) is not None and np.array_equal(h, M.QUAL_CLASS[q])
    assert ctx.quality_remap(q[:0]).shape[0] == 0


def same_qual(got, want):
    recs, hist = got
    w_recs, w_hist = want
    for name in ("n_class", "sum_q", "min_q", "max_q", "median_class"):
        assert np.array_equal(recs[name], w_recs[name]), name
    assert np.array_equal(hist, w_hist)


def test_read_qual_stats(ctx):
    import torch
    from kmerutils_amd import quality
    edges = np.array([0x00, 0x24, 0x25, 0x27, 0x28, 0x36, 0x37, 0x38, 0xFF], np.uint8)
    rng = np.random.default_rng(9)
    reads = [rng.choice(edges, n) for n in (0, 1, 16, 17, 1024, 1025)]
    reads += [edges, np.array([0x21, 0x21, 0x30, 0x30], np.uint8), np.array([0x21, 0x30, 0x30], np.uint8), rng.integers(0, 256, 40_000).astype(np.uint8)]
    quals = np.concatenate(reads)
    off = np.concatenate([[0], np.cumsum([r.size for r in reads])]).astype(np.uint64)
    want = M.read_qual_stats(quals, off)
    assert want[0]["median_class"][7] == 0 and want[0]["median_class"][8] == 4  # a median exactly on a class boundary, and just past it
    assert (want[0]["min_q"][0], want[0]["max_q"][0]) == (0xFF, 0)
    same_qual(ctx.read_qual_stats(quals, off), want)
    pad = np.zeros(quals.size + 64, np.uint8)
    pad[:quals.size] = quals
    d_recs, d_hist = ctx.read_qual_stats(torch.from_numpy(pad).cuda()[:quals.size], torch.from_numpy(off.view(np.int64)).cuda())
    same_qual((d_recs.cpu().numpy().view(QUAL).reshape(-1), d_hist.cpu().numpy().view(np.uint64)), want)
    same_qual(quality.read_quality_stats(quals, off, ctx=ctx), want)
    for names in (("reads",), ("hist",), ()):
        recs, hist = ctx.read_qual_stats(quals, off, want=names)
        assert (recs is not None) == ("reads" in names) and (hist is not None) == ("hist" in names)
        same_qual((want[0] if recs is None else recs, want[1] if hist is None else hist), want)
    recs, hist = ctx.read_qual_stats(quals[:0], np.zeros(1, np.uint64))
    assert recs.shape[0] == 0 and not hist.any()


def test_load_quality_classes(ctx):
    from kmerutils_amd import quality
    text = fastq(records())
    _, quals, off, index = M.ingest_fastq_qual(text)
    got = quality.load_quality_classes(text, ctx)
    assert [q.read_num for q in got] == index.tolist() and [len(q) for q in got] == np.diff(off.astype(np.int64)).tolist()
    assert all(np.array_equal(q.qseq, M.QUAL_CLASS[quals[int(off[i]):int(off[i + 1])]]) for i, q in enumerate(got))

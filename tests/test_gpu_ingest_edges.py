"""The ingest (kmu_ingest.hip) on texts whose line ends fall on the edges of its walk and of its scans: a line end on the last and
first byte of a lane's 16-byte chunk, of a wave's 1 024-byte step and of a 16 384-byte region; texts that end on such an edge; record
and line counts around 1 024, 8 192 and 32 768 (the loop of the single-workgroup scan, a tile of the tiled one, the threshold between
the two); bytes one bit away from '\\n'; a '\\r' that ends the text.  Exact equality with the oracle's reader, and with
read_stats_model.ingest_fastq_qual for the quality bytes.  tests/test_ingest_texts.py checks the texts themselves on the CPU."""
import ctypes as C

import numpy as np
import pytest

import ingest_texts as T
import read_stats_model as M
from kmerutils_amd import _abi as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from kmerutils_amd import lib
    c = lib.Context()
    yield c
    c.close()


def info_dict(info):
    return {k: int(getattr(info, k)) for k in T.INFO_NAMES}


def to_device(text):
    """the text in a device array of exactly its length"""
    import torch
    return torch.from_numpy(np.frombuffer(text, np.uint8).copy()).cuda()


def host(x, dtype):
    return x.cpu().numpy().view(dtype) if hasattr(x, "cpu") else np.asarray(x)


def differs(got, want):
    """what of (bases, offsets, info, record_index) differs from the oracle's; empty when all is equal"""
    bases, offs, info, idx = got
    wb, wo, winfo, widx = want
    out = [] if info_dict(info) == winfo else ["info %r != %r" % (info_dict(info), winfo)]
    for name, g, w in (("bases", host(bases, np.uint8), wb), ("offsets", host(offs, np.uint64), wo), ("record_index", host(idx, np.uint32), widx)):
        if not np.array_equal(g, w):
            out.append(name)
    return out


def check_text(ctx, oracle, text, fmt, device=True):
    """every entry point for the format on one text -> the list of differences"""
    want = getattr(oracle, "ingest_" + fmt)(text)
    bad = []
    host_got = getattr(ctx, "ingest_" + fmt)(text, want_index=True)
    bad += ["host " + d for d in differs(host_got, want)]
    if fmt == "fastq":
        model = M.ingest_fastq_qual(text)
        bases, quals, offs, info, idx = ctx.ingest_fastq_qual(text, want_index=True)
        bad += ["qual " + d for d in differs((bases, offs, info, idx), want)]
        if not (np.array_equal(bases, host_got[0]) and np.array_equal(offs, host_got[1]) and info_dict(info) == info_dict(host_got[2])
                and np.array_equal(idx, host_got[3])):
            bad.append("the call with qualities differs from the call without")
        if not np.array_equal(quals, model[1]):
            bad.append("quality bytes")
    if device:
        got = ctx.ingest_fastx(to_device(text), want_index=True)  # the outputs stay on the device until `differs` reads them
        ctx.synchronize()
        bad += ["device " + d for d in differs(got, want)]
    return bad


@pytest.mark.parametrize("line", T.FASTQ_LINES, ids=["header", "sequence", "separator", "quality"])
def test_fastq_line_end_on_an_edge(ctx, oracle, line):
    bad = {(P, nl, fin): d for P, nl, fin, text in T.placed_texts("fastq", line) for d in [check_text(ctx, oracle, text, "fastq")] if d}
    assert not bad


@pytest.mark.parametrize("what", T.FASTA_LINES)
def test_fasta_line_end_on_an_edge(ctx, oracle, what):
    bad = {(P, nl, fin): d for P, nl, fin, text in T.placed_texts("fasta", what) for d in [check_text(ctx, oracle, text, "fasta")] if d}
    assert not bad


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_text_that_ends_on_an_edge(ctx, oracle, fmt):
    bad = {}
    for n_bytes in T.END_SIZES:
        for nl in T.LINE_ENDS:
            for fin in (True, False):
                d = check_text(ctx, oracle, T.end_at(n_bytes, fmt, fin, nl), fmt)
                if d:
                    bad[n_bytes, nl, fin] = d
    assert not bad


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_record_counts_on_the_scan_edges(ctx, oracle, fmt):
    """FASTQ: n records through the scans of keep flags and kept lengths; FASTA: n lines through the scans of header flags (uint32)
    and line lengths (uint64), and the records they make through the former two"""
    bad = {n: d for n in T.RECORD_COUNTS for d in [check_text(ctx, oracle, T.many_records(n, fmt), fmt, device=False)] if d}
    assert not bad


@pytest.mark.parametrize("name", sorted(T.special_texts()))
def test_special_text(ctx, oracle, name):
    fmt, text = T.special_texts()[name]
    assert not check_text(ctx, oracle, text, fmt)


# ---- errors at edges ----------------------------------------------------------------------------------------------------------
def refused_and_nothing_written(ctx, text, quals=False):
    """the entry point with outputs large enough for the text: KMU_E_BAD_ARG, and the outputs as they were"""
    from kmerutils_amd import lib
    text = np.frombuffer(text, np.uint8)
    bases, quality, offs, idx = np.full(text.size, 7, np.uint8), np.full(text.size, 7, np.uint8), np.full(64, 7, np.uint64), np.full(64, 7, np.uint32)
    info = A.IngestInfo()
    more = (lib._ptr(quality)[0], quality.size) if quals else ()
    entry = ctx.L.kmu_ingest_fastq_qual if quals else ctx.L.kmu_ingest_fastq
    rc = entry(ctx.h, lib._ptr(text)[0], text.size, A.MEM_HOST, lib._ptr(bases)[0], bases.size, *more, lib._ptr(offs)[0], offs.size,
               lib._ptr(idx)[0], C.byref(info))
    return rc == A.E_BAD_ARG and (bases == 7).all() and (quality == 7).all() and (offs == 7).all() and (idx == 7).all()


@pytest.mark.parametrize("nl", T.LINE_ENDS, ids=["lf", "crlf"])
def test_a_wrong_first_byte_on_the_first_byte_of_a_region(ctx, oracle, nl):
    from kmerutils_amd.lib import KmuError
    # the quality line of record 2 ends on the last byte of region 0: the '@' of record 3 opens region 1; likewise the '+' of record 2
    for line, first, other in ((3, b"@", b"x"), (1, b"+", b"-")):
        text = T.place_fastq(T.REGION - 1, line, nl, True)
        assert text[T.REGION:T.REGION + 1] == first
        text = text[:T.REGION] + other + text[T.REGION + 1:]
        with pytest.raises(oracle.OracleError):
            oracle.ingest_fastq(text)
        for quals in (False, True):
            assert refused_and_nothing_written(ctx, text, quals)
        with pytest.raises(KmuError) as e:
            ctx.ingest_fastx(to_device(text))
        assert e.value.code == A.E_BAD_ARG and "invalid record" in str(e.value)
    # FASTA: without its '>' the header of record 3 is a sequence line of record 2, with bytes that are no bases: no error
    text = T.place_fasta(T.REGION - 1, "lastseq", nl, True)
    assert text[T.REGION:T.REGION + 1] == b">"
    text = text[:T.REGION] + b"x" + text[T.REGION + 1:]
    assert oracle.ingest_fasta(text)[2]["n_records"] == 5 and oracle.ingest_fasta(text)[3].tolist() == [0, 4]
    assert not check_text(ctx, oracle, text, "fasta")


@pytest.mark.parametrize("nl", T.LINE_ENDS, ids=["lf", "crlf"])
def test_a_short_quality_line_in_the_region_after_its_sequence(ctx, oracle, nl):
    from kmerutils_amd.lib import KmuError
    text = T.place_fastq(T.REGION - 1, 1, nl, True)  # the sequence line of record 2 ends region 0
    lines = text.split(nl)
    assert len(lines[9]) == len(lines[11]) == 17 and len(nl.join(lines[:10])) == T.REGION - len(nl)
    lines[11] = lines[11][:-1]
    text = nl.join(lines)
    assert M.ingest_fastq_qual(text) is None
    assert refused_and_nothing_written(ctx, text, quals=True)
    with pytest.raises(KmuError) as e:
        ctx.ingest_fastq_qual(to_device(text))
    assert e.value.code == A.E_BAD_ARG and "invalid record" in str(e.value)
    assert not differs(ctx.ingest_fastq(text, want_index=True), oracle.ingest_fastq(text))  # without qualities the line is not looked at


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_misaligned_device_text_is_refused(ctx, oracle, fmt):
    from kmerutils_amd.lib import KmuError
    text = (T.place_fastq if fmt == "fastq" else T.place_fasta)(T.REGION, 1 if fmt == "fastq" else "seq", b"\n", True)
    t = to_device(b"\n" + text)[1:]
    assert t.data_ptr() % 16 == 1
    for call in (ctx.ingest_fastx, getattr(ctx, "ingest_" + fmt)):
        with pytest.raises(KmuError) as e:
            call(t)
        assert e.value.code == A.E_BAD_ARG and "aligned" in str(e.value)
    fresh = t.clone()
    assert fresh.data_ptr() % 16 == 0
    got = ctx.ingest_fastx(fresh, want_index=True)
    ctx.synchronize()
    assert not differs(got, oracle.ingest_fastx(text))

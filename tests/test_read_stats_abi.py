"""The read statistics (kmu_read_stats, kmu_read_qual_stats, kmu_quality_remap, kmu_ingest_fastq_qual, the two layout calls) at the
C-ABI, without a GPU: the library exports the calls, the binding lists them, the records have the layout of the header, the layout
calls answer without a device, and the argument checks that need no device."""
import ctypes as C
import os
import sys

import numpy as np

from kmerutils_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_stats_model as M  # noqa: E402

CALLS = ("kmu_len_hist_layout", "kmu_len_bucket_range", "kmu_read_stats", "kmu_ingest_fastq_qual", "kmu_quality_remap", "kmu_read_qual_stats")


def _lib():
    from kmerutils_amd import build, lib
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return lib.load(), lib


def test_library_exports_the_calls():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "kmu.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in CALLS:
        assert name in lib.SYMBOLS and hasattr(L, name), name
        assert name + "(" in header and name in integration, name
    for m in ("read_stats", "ingest_fastq_qual", "quality_remap", "read_qual_stats"):
        assert callable(getattr(lib.Context, m)), m
    assert callable(lib.len_hist_layout) and callable(lib.len_bucket_range)
    for word in ("kmu_read_comp", "kmu_read_stats_params", "kmu_read_stats_info", "kmu_read_qual"):
        assert "} %s;" % word in header, word


def test_mirrors_carry_the_names():
    from kmerutils_amd import quality, statutils
    for m in ("value_at_quantile", "ascii_dump_acgt_distribution", "ascii_dump_readlen_distribution"):
        assert callable(getattr(statutils.ReadBaseDistribution, m)), m
    assert callable(statutils.get_base_count_par)
    for name in ("remap_quality8", "quality_to_proba", "QSequenceRaw", "load_quality_classes", "read_quality_stats"):
        assert callable(getattr(quality, name)), name
    hpp = open(os.path.join(ROOT, "include", "kmerutils.hpp")).read()
    for word in ("class ReadBaseDistribution", "get_base_count_par(", "ascii_dump_acgt_distribution(", "ascii_dump_readlen_distribution(",
                 "value_at_quantile(", "remap_quality8(", "ingest_fastq_qual(", "read_quality_stats(", "std::to_chars"):
        assert word in hpp, word
    for tool in ("parsefastq.py", os.path.join("tools", "parsefastq.cpp")):
        src = open(os.path.join(ROOT, "kmerutils_amd", tool)).read()
        assert "--stats" in src and "bases.histo" in src and "readlen.histo" in src and "quality.histo" in src, tool


def same_layout(struct, dtype, size):
    dt = np.dtype(dtype)
    assert C.sizeof(struct) == size == dt.itemsize
    assert [name for name, _ in struct._fields_] == list(dt.names)
    for name, _ in struct._fields_:
        assert dt.fields[name][1] == getattr(struct, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(struct, name).size, name


def test_record_layouts():
    same_layout(A.ReadComp, A.READ_COMP_DTYPE, 48)
    same_layout(A.ReadStatsInfo, A.READ_STATS_INFO_DTYPE, 96)
    same_layout(A.ReadQual, A.READ_QUAL_DTYPE, 80)
    assert C.sizeof(A.ReadStatsParams) == 16
    assert [(n, getattr(A.ReadStatsParams, n).offset) for n, _ in A.ReadStatsParams._fields_] == [("sig_digits", 0), ("flags", 4), ("max_len", 8)]
    assert [(n, getattr(A.ReadComp, n).offset) for n, _ in A.ReadComp._fields_] == [("n_base", 0), ("n_other", 32), ("pct", 40), ("len_bucket", 44)]
    assert [(n, getattr(A.ReadQual, n).offset) for n, _ in A.ReadQual._fields_] == [
        ("n_class", 0), ("sum_q", 64), ("min_q", 72), ("max_q", 73), ("median_class", 74), ("pad", 75)]
    assert [getattr(A.ReadStatsInfo, n).offset for n in A.READ_STATS_INFO] == [0, 8, 16, 48, 56, 64, 72, 80, 88]


def test_layout_calls_answer_without_a_device():
    _, lib = _lib()
    assert lib.len_hist_layout(1_000_000, 3) == (11_264, 1_048_576)
    for max_len in (1, 31, 32, 63, 64, 5000, 1_000_000, 1 << 40):
        for sig in range(1, 6):
            assert lib.len_hist_layout(max_len, sig) == M.layout(max_len, sig), (max_len, sig)
    for sig in range(1, 6):
        n_buckets, _ = M.layout(1 << 30, sig)
        for bucket in list(range(0, 100)) + list(range(n_buckets - 100, n_buckets)) + [1 << (M.SUB_BITS[sig] - 1), 1 << M.SUB_BITS[sig], 3 << (M.SUB_BITS[sig] - 1)]:
            assert lib.len_bucket_range(sig, bucket) == M.bucket_range(bucket, sig), (sig, bucket)


def test_bad_arguments_are_bad_arg_and_write_nothing():
    L, _ = _lib()
    vp = C.c_void_p
    n, limit = C.c_uint32(7), C.c_uint64(7)
    for max_len, sig in ((0, 3), (1000, 0), (1000, 6), (1000, -1)):
        assert L.kmu_len_hist_layout(max_len, sig, C.byref(n), C.byref(limit)) == A.E_BAD_ARG and (n.value, limit.value) == (7, 7)
    assert L.kmu_len_hist_layout(1000, 3, None, C.byref(limit)) == A.E_BAD_ARG and L.kmu_len_hist_layout(1000, 3, C.byref(n), None) == A.E_BAD_ARG
    lo, hi = C.c_uint64(7), C.c_uint64(7)
    for sig in (0, 6):
        assert L.kmu_len_bucket_range(sig, 5, C.byref(lo), C.byref(hi)) == A.E_BAD_ARG and (lo.value, hi.value) == (7, 7)
    assert L.kmu_len_bucket_range(3, 5, None, C.byref(hi)) == A.E_BAD_ARG and hi.value == 7
    # no context: refused before anything is looked at
    bases = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()
    off = np.array([0, 16], np.uint64)
    comp = np.full(48, 7, np.uint8)
    pct, hist = np.full(404, 7, np.uint64), np.full(11264, 7, np.uint64)
    info = A.ReadStatsInfo()
    info.n_reads = 7
    p = A.ReadStatsParams(3, 0, 1_000_000)
    rc = L.kmu_read_stats(None, C.byref(p), bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST, comp.ctypes.data_as(vp),
                          pct.ctypes.data_as(vp), hist.ctypes.data_as(vp), C.byref(info))
    assert rc == A.E_BAD_ARG and (comp == 7).all() and (pct == 7).all() and (hist == 7).all() and info.n_reads == 7
    out = np.full(16, 7, np.uint8)
    assert L.kmu_quality_remap(None, bases.ctypes.data_as(vp), 16, A.MEM_HOST, out.ctypes.data_as(vp)) == A.E_BAD_ARG and (out == 7).all()
    recs, chist = np.full(80, 7, np.uint8), np.full(8, 7, np.uint64)
    rc = L.kmu_read_qual_stats(None, bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST, recs.ctypes.data_as(vp), chist.ctypes.data_as(vp))
    assert rc == A.E_BAD_ARG and (recs == 7).all() and (chist == 7).all()
    text = np.frombuffer(b"@r\nACGT\n+\nIIII\n", np.uint8).copy()
    ing = A.IngestInfo()
    ing.n_records = 7
    rc = L.kmu_ingest_fastq_qual(None, text.ctypes.data_as(vp), text.size, A.MEM_HOST, None, 0, None, 0, None, 0, None, C.byref(ing))
    assert rc == A.E_BAD_ARG and ing.n_records == 7
    assert A.RS_PCT_ROWS == 101 and A.RS_QUAL_CLASSES == 8 and A.RS_NO_BUCKET == 0xFFFFFFFF

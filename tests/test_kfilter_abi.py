"""The count prefilter (kmu_kfilter_*, kmu_count_add_reads_filtered) at the C-ABI, without a GPU: the library exports the calls, the
binding lists them, the records have the layout of the header, and the argument checks that need no device answer."""
import ctypes as C
import os

import numpy as np

from kmerutils_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("kmu_kfilter_cells_for", "kmu_kfilter_create", "kmu_kfilter_destroy", "kmu_kfilter_reset", "kmu_kfilter_add_reads",
         "kmu_kfilter_add_kmers", "kmu_kfilter_query", "kmu_kfilter_info", "kmu_kfilter_export", "kmu_kfilter_merge",
         "kmu_kfilter_select_reads", "kmu_count_add_reads_filtered")


def _lib():
    from kmerutils_amd import build, lib
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return lib.load(), lib


def test_library_exports_the_prefilter_calls():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "kmu.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in CALLS:
        assert name in lib.SYMBOLS and hasattr(L, name), name
        assert name + "(" in header and name in integration, name
    for m in ("reset", "add_reads", "add_kmers", "query", "info", "export", "merge", "select_reads"):
        assert callable(getattr(lib.KFilter, m)), m
    assert callable(lib.Context.kfilter) and callable(lib.Counter.add_reads_filtered)


def test_mirrors_carry_the_names():
    from kmerutils_amd import kmercount
    for m in ("insert_reads", "insert_kmer", "seen_class", "info", "merge", "words"):
        assert callable(getattr(kmercount.KmerPrefilter, m)), m
    assert callable(kmercount.count_repeated_kmers) and callable(kmercount.KmerCounter.insert_reads_filtered)
    hpp = open(os.path.join(ROOT, "include", "kmerutils.hpp")).read()
    for word in ("class KmerPrefilter", "count_repeated_kmers(", "insert_reads_filtered(", "seen_class(", "insert_kmer(Kmer kmer)",
                 "words()", "merge(const KmerPrefilter"):
        assert word in hpp, word
    for tool in ("parsefastq.py", os.path.join("tools", "parsefastq.cpp")):
        src = open(os.path.join(ROOT, "kmerutils_amd", tool)).read()
        assert "--repeated" in src and "--filter-bits" in src, tool


def test_record_layouts():
    assert C.sizeof(A.KFilterInfo) == 56 and C.sizeof(A.KFilterParams) == 24
    dt = np.dtype(A.KFILTER_INFO_DTYPE)
    assert dt.itemsize == 56
    assert [name for name, _ in A.KFilterInfo._fields_] == list(dt.names)
    for name, _ in A.KFilterInfo._fields_:
        assert dt.fields[name][1] == getattr(A.KFilterInfo, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(A.KFilterInfo, name).size, name
    assert [(n, getattr(A.KFilterParams, n).offset) for n, _ in A.KFilterParams._fields_] == [
        ("kmer_type", 0), ("kmer_size", 4), ("n_hashes", 8), ("flags", 12), ("n_cells", 16)]


def test_null_arguments_are_bad_arg_and_write_nothing():
    L, _ = _lib()
    vp = C.c_void_p
    keys = np.arange(8, dtype=np.uint64)
    cls = np.full(8, 7, np.uint8)
    assert L.kmu_kfilter_query(None, keys.ctypes.data_as(vp), 8, A.MEM_HOST, cls.ctypes.data_as(vp)) == A.E_BAD_ARG
    assert (cls == 7).all()
    assert L.kmu_kfilter_add_kmers(None, keys.ctypes.data_as(vp), 8, A.MEM_HOST) == A.E_BAD_ARG
    assert L.kmu_kfilter_reset(None) == A.E_BAD_ARG
    bases = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGTACGTACGT", np.uint8).copy()
    off = np.array([0, 36], np.uint64)
    assert L.kmu_kfilter_add_reads(None, bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST) == A.E_BAD_ARG
    info = A.KFilterInfo()
    info.n_added = 7
    assert L.kmu_kfilter_info(None, C.byref(info)) == A.E_BAD_ARG and info.n_added == 7
    words = np.full(4, 7, np.uint64)
    assert L.kmu_kfilter_export(None, words.ctypes.data_as(vp), A.MEM_HOST) == A.E_BAD_ARG and (words == 7).all()
    assert L.kmu_kfilter_merge(None, None) == A.E_BAD_ARG
    out = np.full(8, 7, np.uint64)
    n = C.c_uint64(7)
    rc = L.kmu_kfilter_select_reads(None, bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST, out.ctypes.data_as(vp), 8, C.byref(n))
    assert rc == A.E_BAD_ARG and (out == 7).all() and n.value == 7
    # a counter without a filter, a filter without a counter: both NULL here, nothing to tell apart without a device
    rc = L.kmu_count_add_reads_filtered(None, None, bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST, C.byref(n))
    assert rc == A.E_BAD_ARG and n.value == 7
    L.kmu_kfilter_destroy(None)  # (a no-op)


def test_create_refuses_before_any_device_work():
    """no context, no parameters, no place for the handle; and the parameter ranges, stated here with no context to allocate in"""
    L, _ = _lib()
    h = C.c_void_p(0x5A5A)
    good = A.KFilterParams(A.KMER64BIT, 31, 4, 0, 1000)
    assert L.kmu_kfilter_create(None, C.byref(good), C.byref(h)) == A.E_BAD_ARG and h.value == 0x5A5A
    for n_hashes, n_cells in ((0, 1000), (9, 1000), (4, 0)):
        p = A.KFilterParams(A.KMER64BIT, 31, n_hashes, 0, n_cells)
        assert L.kmu_kfilter_create(None, C.byref(p), C.byref(h)) == A.E_BAD_ARG and h.value == 0x5A5A
    assert A.KFILTER_MAX_HASHES == 8 and A.KFILTER_MAX_CELLS == (1 << 32) - 1

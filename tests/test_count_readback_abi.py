"""kmu_count_histogram / kmu_count_read_profile at the C-ABI, without a GPU: the library exports them, the binding lists them,
the record has the layout of the header, and the argument checks that need no device answer."""
import ctypes as C

import numpy as np

from kmerutils_amd import _abi as A


def _lib():
    from kmerutils_amd import build, lib
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return lib.load(), lib


def test_library_exports_the_readback_calls():
    L, lib = _lib()
    for name in ("kmu_count_histogram", "kmu_count_read_profile"):
        assert name in lib.SYMBOLS
        assert hasattr(L, name)
    assert callable(getattr(lib.Counter, "histogram")) and callable(getattr(lib.Counter, "read_profile"))


def test_mirrors_have_the_readback_methods():
    import os
    from kmerutils_amd import kmercount
    assert callable(getattr(kmercount.KmerCounter, "get_count_histogram"))
    assert callable(getattr(kmercount.KmerCounter, "get_reads_abundance"))
    hpp = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmerutils.hpp")).read()
    assert "get_count_histogram()" in hpp and "get_reads_abundance(" in hpp


def test_null_counter_is_bad_arg_and_writes_nothing():
    L, _ = _lib()
    vp = C.c_void_p
    hist = np.full(256, 7, np.uint64)
    assert L.kmu_count_histogram(None, hist.ctypes.data_as(vp), 256, A.MEM_HOST) == A.E_BAD_ARG
    assert (hist == 7).all()
    bases = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()
    off = np.array([0, 16], np.uint64)
    counts = np.full(16, 7, np.uint16)
    stats = np.zeros(1, np.dtype(A.READ_ABUNDANCE_DTYPE))
    stats["n_kmers"] = 7
    rc = L.kmu_count_read_profile(None, bases.ctypes.data_as(vp), off.ctypes.data_as(vp), 1, A.MEM_HOST, 2, counts.ctypes.data_as(vp),
                                  stats.ctypes.data_as(vp))
    assert rc == A.E_BAD_ARG
    assert (counts == 7).all() and stats["n_kmers"][0] == 7


def test_record_layout():
    assert C.sizeof(A.ReadAbundance) == 32
    dt = np.dtype(A.READ_ABUNDANCE_DTYPE)
    assert dt.itemsize == 32
    assert [name for name, _ in A.ReadAbundance._fields_] == list(dt.names)
    for name, _ in A.ReadAbundance._fields_:
        assert dt.fields[name][1] == getattr(A.ReadAbundance, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(A.ReadAbundance, name).size, name


def test_counter_closes_at_the_end_of_a_with_block():
    """Counter has the life cycle of the other handles: `with` closes it once, and a close after the context's is silent"""
    import types
    from kmerutils_amd import lib
    freed = []
    ctx = types.SimpleNamespace(h=1, L=types.SimpleNamespace(kmu_count_destroy=freed.append))
    counter = object.__new__(lib.Counter)
    counter.ctx, counter.L, counter.h = ctx, ctx.L, 7
    with counter as same:
        assert same is counter and not freed
    assert counter.h is None and freed == [7]
    counter.close()
    counter.h, ctx.h = 8, None
    counter.close()
    assert counter.h is None and freed == [7]

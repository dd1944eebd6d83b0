"""kmu_sketch_groups at the C-ABI, without a GPU: the library exports it, the binding lists it, and the argument checks that
need no device answer."""
import ctypes as C

import numpy as np

from kmerutils_amd import _abi as A


def _lib():
    from kmerutils_amd import build, lib
    build.build()  # hipcc cross-compiles gfx950 without a GPU
    return lib.load(), lib


def test_library_exports_sketch_groups():
    L, lib = _lib()
    assert "kmu_sketch_groups" in lib.SYMBOLS
    assert hasattr(L, "kmu_sketch_groups")
    assert hasattr(lib.Context, "sketch_groups")


def test_null_context_is_bad_arg():
    L, _ = _lib()
    p = A.SketchParams(A.ALGO_PROB3A, A.KMER32BIT, 8, 16, A.SIG_U32, 0, A.FHASH_CANON_INVHASH, 0, A.MODE_ALL_SEQS, 0, 0, 0)
    bases = np.frombuffer(b"ACGTACGTACGTACGT", np.uint8).copy()
    off = np.array([0, 16], np.uint64)
    go = np.array([0, 1], np.uint64)
    out = np.zeros((1, 16), np.uint32)
    vp = C.c_void_p
    rc = L.kmu_sketch_groups(None, C.byref(p), bases.ctypes.data_as(vp), off.ctypes.data_as(vp), None, 1, go.ctypes.data_as(vp), 1,
                             out.ctypes.data_as(vp))
    assert rc == A.E_BAD_ARG
    assert not out.any()


def test_mirrors_have_the_grouped_call():
    from kmerutils_amd import sketching
    for cls in (sketching.ProbHash3aSketch, sketching.SuperHashSketch, sketching.SuperHash2Sketch, sketching.OptDensHashSketch,
                sketching.RevOptDensHashSketch, sketching.HyperLogLogSketch):
        assert callable(getattr(cls, "sketch_compressedkmer_seqs_groups"))

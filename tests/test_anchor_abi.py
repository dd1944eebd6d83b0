"""-m "not gpu": the host side of the read anchors -- kmu_anchor_layout (plain host C), the Python mirror of the reference's
names, the inverse index, and the three properties of the oracle that tests/test_gpu_anchors.py builds its expected rows on."""
import ctypes as C

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import anchor, lib


def _layout(off, window, overlap):
    L = lib.load()
    off = np.asarray(off, np.uint64)
    out = np.full(off.size, 77, np.uint64)
    rc = L.kmu_anchor_layout(off.ctypes.data_as(C.c_void_p), off.size - 1, window, overlap, out.ctypes.data_as(C.c_void_p))
    return rc, out.tolist()


def test_anchor_layout_host_only():
    assert _layout([0, 10, 1010, 3011], 1000, 250) == (0, [0, 1, 3, 6])  # ceil(L / 750): 10 -> 1, 1000 -> 2, 2001 -> 3
    assert _layout([0, 0, 5], 4, 1) == (0, [0, 0, 2])                    # L = 0: no slice
    assert _layout([5, 5], 4, 1)[0] == 0
    assert _layout([0, 10], 1000, 1000)[0] == A.E_BAD_ARG                # overlap == window
    assert _layout([0, 10], 0, 0)[0] == A.E_BAD_ARG                      # window == 0
    assert _layout([0, 10], 5, 9)[0] == A.E_BAD_ARG
    with pytest.raises(lib.KmuError) as e:
        lib.anchor_layout(np.array([0, 10], np.uint64), 8, 8)
    assert e.value.code == A.E_BAD_ARG
    assert lib.anchor_layout(np.array([0, 10, 1010, 3011], np.uint64), 1000, 250).tolist() == [0, 1, 3, 6]


def test_constants_match_the_header():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "kmu.h")).read()
    assert int(re.search(r"#define KMU_ANCHOR_MAX_NBKMER (\d+)", txt).group(1)) == A.ANCHOR_MAX_NBKMER >= 256
    assert int(re.search(r"#define KMU_ANCHOR_TILE_KMERS (\d+)", txt).group(1)) == A.ANCHOR_TILE_KMERS


def test_anchors_generator_parameters():
    p = anchor.AnchorsGeneratorParameters("reads.fasta", 1000, 16, 21, 250)
    assert (p.get_fasta_name(), p.get_window(), p.get_nbkmer(), p.get_kmer_size(), p.get_overlap()) == ("reads.fasta", 1000, 16, 21, 250)
    assert p.get_stride() == 750
    sp = p.sketch_params()
    assert (sp.algo, sp.kmer_type, sp.kmer_size, sp.sketch_size, sp.sig_type) == (A.ALGO_BOTTOMK, A.KMER64BIT, 21, 16, A.SIG_U64)
    assert (sp.hasher, sp.fhash, sp.block_size) == (A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED, 0)
    assert anchor.AnchorsGeneratorParameters("x", 100, 4, 16, 0).sketch_params().kmer_type == A.KMER16B32BIT
    assert anchor.AnchorsGeneratorParameters("x", 100, 4, 11, 0).sketch_params(fhash=A.FHASH_CANON_VALUE).kmer_type == A.KMER32BIT
    with pytest.raises(ValueError):
        anchor.AnchorsGeneratorParameters("x", 100, 4, 15, 0).sketch_params()


def test_anchors_by_minhash_and_views():
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    # two reads: read 0 has rows 0..2 (the last one empty), read 1 has row 3; rows 0 and 3 share their smallest hash
    hashes = np.array([[5, 9, M], [7, M, M], [M, M, M], [5, 6, 8]], np.uint64)
    counts = np.array([[1, 2, 0], [3, 0, 0], [0, 0, 0], [1, 1, 255]], np.uint32)
    n = np.array([2, 1, 0, 3], np.uint32)
    rows = np.array([0, 3, 4], np.uint64)
    idx = anchor.anchors_by_minhash(hashes, n, rows, stride=30, first_readnum=10)
    assert idx == {5: [(10, 0), (11, 0)], 7: [(10, 30)]}
    p = anchor.AnchorsGeneratorParameters("x", 40, 3, 11, 10)
    ra = anchor.ReadAnchors(p, 10, hashes, counts, n, 0, 3)
    assert ra.get_nb_slice() == 3 and len(ra) == 3
    assert [(s.readnum, s.slicepos) for s in ra.anchors] == [(10, 0), (10, 30), (10, 60)]
    assert ra[0].minhash == [(5, 1), (9, 2)] and ra[1].minhash == [(7, 3)] and ra[2].minhash == []
    assert ra[0].get_minhash_key() == 5
    with pytest.raises(IndexError):
        ra[2].get_minhash_key()


# ---- what the GPU tests take from the oracle ----------------------------------------------------------------------------
def _bk(k, m, hasher, fhash, kmer_type=A.KMER64BIT):
    return A.SketchParams(A.ALGO_BOTTOMK, kmer_type, k, m, A.SIG_U64, hasher, fhash, 0, A.MODE_PER_SEQ, A.INPUT_ASCII, A.MEM_HOST, 0)


def test_oracle_short_substring_is_all_padding(oracle):
    bases, off = oracle.concat([b"ACGTACGTAC", b"A"])
    sig, cnt = oracle.sketch(bases, off, _bk(21, 4, A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED), want_counts=True)
    assert (sig == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (cnt == 0).all()


def test_oracle_int64hash_counts_wrap_at_256(oracle):
    k = 21
    for nk, want in ((255, 255), (256, 0), (301, 45)):
        bases, off = oracle.concat([b"A" * (nk + k - 1)])
        sig, cnt = oracle.sketch(bases, off, _bk(k, 4, A.HASHER_INT64HASH, A.FHASH_VALUE_MASKED), want_counts=True)
        assert cnt[0].tolist() == [want, 0, 0, 0] and sig[0, 0] != np.uint64(0xFFFFFFFFFFFFFFFF) and sig[0, 1] == np.uint64(0xFFFFFFFFFFFFFFFF)
        sig, cnt = oracle.sketch(bases, off, _bk(k, 4, A.HASHER_NOHASH, A.FHASH_CANON_INVHASH), want_counts=True)
        assert cnt[0].tolist() == [nk, 0, 0, 0]  # u16 counts: no wrap at these sizes


def test_oracle_range_is_the_kmers_of_the_substring(oracle):
    rng = np.random.default_rng(5)
    s = bytes(rng.choice(list(b"ACGT"), size=300).astype(np.uint8))
    k, b, e = 21, 37, 211
    bases, off = oracle.concat([s])
    full = oracle.kmer_hashes_range(bases, off, A.KMER64BIT, k, A.FHASH_VALUE_MASKED, [b], [e])
    sb, so = oracle.concat([s[b:e]])
    sub = oracle.kmer_hashes(sb, so, A.KMER64BIT, k, A.FHASH_VALUE_MASKED)
    assert np.array_equal(full[b:e - k + 1], sub[:e - b - k + 1])

"""The count prefilter's definition (include/kmu.h, restated in tests/kfilter_model.py) on the CPU: the planes are a function of
the multiset of occurrences, no key added twice is missed, and the hash spreads keys well enough to be of use."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfilter_model as M  # noqa: E402


def _keys(n, seed):
    """n distinct values below 2^62 (canonical compressed 31-mers look like that)"""
    v = np.unique(np.random.default_rng(seed).integers(0, 1 << 62, int(n * 1.01) + 16, dtype=np.uint64))
    return np.random.default_rng(seed + 1).permutation(v)[:n]


def test_planes_depend_on_the_multiset_only():
    keys = _keys(3000, 1)
    occ = np.concatenate([keys, keys[:700], keys[:200], keys[100:130]])  # counts 1 .. 4
    rng = np.random.default_rng(2)
    for n_cells, n_hashes in ((1, 1), (8, 8), (1000, 4), (M.cells_for(3000, 16), 4), (1021, 3)):
        whole = M.build(occ, n_cells, n_hashes)
        perm = M.build(rng.permutation(occ), n_cells, n_hashes)
        assert np.array_equal(whole[0], perm[0]) and np.array_equal(whole[1], perm[1]), (n_cells, n_hashes)
        # three builds of a split of the permuted input, merged together
        sh = rng.permutation(occ)
        parts = [M.build(p, n_cells, n_hashes) for p in (sh[:1000], sh[1000:1001], sh[1001:])]
        m = M.merge(M.merge(parts[0], parts[1]), parts[2])
        assert np.array_equal(whole[0], m[0]) and np.array_equal(whole[1], m[1]), (n_cells, n_hashes)
        # continuing a build is building the whole
        cont = M.build(occ[2000:], n_cells, n_hashes, planes=M.build(occ[:2000], n_cells, n_hashes))
        assert np.array_equal(whole[0], cont[0]) and np.array_equal(whole[1], cont[1])
        assert (whole[1] & ~whole[0]).max() == 0  # plane B lies inside plane A


def test_no_false_negatives():
    keys = _keys(5000, 3)
    twice, once, never = keys[:1500], keys[1500:4000], keys[4000:]
    occ = np.random.default_rng(4).permutation(np.concatenate([twice, twice, twice[:300], once]))
    for n_cells, n_hashes in ((1, 1), (8, 8), (1000, 4), (M.cells_for(4000, 16), 4)):
        planes = M.build(occ, n_cells, n_hashes)
        assert (M.classes(planes, twice, n_hashes) == 2).all()      # added at least twice: always class 2
        assert (M.classes(planes, once, n_hashes) >= 1).all()       # added once: 1, or 2 by collision
        cn = M.classes(planes, never, n_hashes)
        a, _ = planes
        cell, mask = M.cell_mask(never, n_cells, n_hashes)
        # never added: class 0 unless every bit of the mask was set by others -- never class 1 or 2 with a bit missing in A
        assert np.array_equal(cn == 0, (a[cell] & mask) != mask)
    # at a useful size nearly every key that was never added is class 0
    assert (M.classes(M.build(occ, M.cells_for(4000, 16), 4), never, 4) == 0).mean() > 0.97


def test_mask_and_cell_ranges():
    keys = _keys(20000, 5)
    for n_cells in (1, 3, 1000, (1 << 32) - 1):
        for n_hashes in (1, 4, 8):
            cell, mask = M.cell_mask(keys, n_cells, n_hashes)
            assert int(cell.max()) < n_cells
            bits = np.unpackbits(mask.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)
            assert bits.min() >= 1 and bits.max() <= n_hashes  # coinciding positions collapse
    assert M.sm(np.array([0], np.uint64))[0] == 0xE220A8397B1DCDAF  # splitmix64: the first output of seed 0


def test_cells_for_edges():
    from kmerutils_amd import build, lib
    build.build()  # (plain host code of the library: no device)
    f = lib.kfilter_cells_for
    assert f(0, 16) == 1 and f(1, 1) == 1 and f(4, 16) == 1 and f(5, 16) == 2 and f(64, 1) == 1 and f(65, 1) == 2
    assert f(100_000 + 10_000, 16) == 27_500
    top = (1 << 32) - 1
    assert f(top * 4, 16) == top and f(top * 4 + 1, 16) == 0  # the largest filter, and one cell more
    assert f(1 << 63, 16) == 0 and f((1 << 64) - 1, 0xFFFFFFFF) == 0  # products beyond 2^64 do not wrap into range
    assert f(7, 0) == 1
    for e, b in ((0, 16), (5, 16), (110_000, 16), (top * 4, 16), (top * 4 + 1, 16), (12345, 7)):
        assert f(e, b) == M.cells_for(e, b)


def test_est_distinct_formula():
    assert M.est_distinct(10, 4, 0) == 0.0 and math.isinf(M.est_distinct(10, 4, 640))
    keys = _keys(50_000, 6)
    n_cells = M.cells_for(keys.size, 16)
    a, _ = M.build(keys, n_cells, 4)
    # The formula takes a key for n_hashes bits; positions that coincide inside the 64-bit cell collapse, so a key sets
    # 64 (1 - (63/64)^4) = 3.907 bits on average and the estimate reads 2.3 % low.  Around that: the spread of 50 000 keys.
    ratio = M.est_distinct(n_cells, 4, M.popcount(a)) / keys.size
    assert abs(ratio - 64 * (1 - (63 / 64) ** 4) / 4) < 0.01


def test_singletons_rarely_pass():
    """the guard on the definition itself: with a useless hash every other test would still pass bit for bit.  100 000 singletons
    and 10 000 keys added twice at 16 bits per distinct key and 4 hashes: 0.50 % of the singletons are class 2 (the Bloom rate of
    plane A); the bound is 2 %."""
    keys = _keys(110_000, 7)
    once, twice = keys[:100_000], keys[100_000:]
    n_cells = M.cells_for(keys.size, 16)
    assert n_cells == 27_500
    planes = M.build(np.concatenate([once, twice, twice]), n_cells, 4)
    assert (M.classes(planes, twice, 4) == 2).all()
    share = float((M.classes(planes, once, 4) == 2).mean())
    print("singletons in class 2: %.4f" % share)
    assert share < 0.02

"""The count prefilter (kmu_kfilter, include/kmu.h) restated in numpy: a helper for the tests, not a test.

The filter is n_cells cells {uint64 A, uint64 B}.  build() adds the occurrences ONE AFTER THE OTHER, exactly as the header states
the update of one occurrence; the device adds them concurrently with atomics and must arrive at the same planes."""
import math

import numpy as np

M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def sm(z):
    """splitmix64's output function over the next state, modulo 2^64, on a uint64 array"""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z += np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def cell_mask(v, n_cells, n_hashes):
    """(cell uint64 [n], mask uint64 [n]) of the keys v"""
    assert 1 <= n_cells <= (1 << 32) - 1 and 1 <= n_hashes <= 8
    h = sm(np.atleast_1d(np.asarray(v, np.uint64)))
    g = sm(h)
    cell = ((h >> np.uint64(32)) * np.uint64(n_cells)) >> np.uint64(32)  # (both factors below 2^32: no wrap)
    mask = np.zeros(h.size, np.uint64)
    for i in range(n_hashes):
        mask |= np.uint64(1) << ((g >> np.uint64(6 * i)) & np.uint64(63))
    return cell, mask


def build(occurrences, n_cells, n_hashes, planes=None):
    """the planes (A uint64 [n_cells], B uint64 [n_cells]) after adding the occurrences one by one, in the order given"""
    cell, mask = cell_mask(occurrences, n_cells, n_hashes) if len(occurrences) else (np.zeros(0, np.uint64), np.zeros(0, np.uint64))
    a = [0] * n_cells if planes is None else [int(x) for x in planes[0]]
    b = [0] * n_cells if planes is None else [int(x) for x in planes[1]]
    for c, m in zip(cell.tolist(), mask.tolist()):
        old = a[c]
        a[c] = old | m
        rep = old & m
        if rep:
            b[c] |= rep
    return np.array(a, np.uint64), np.array(b, np.uint64)


def words(planes):
    """A0 B0 A1 B1 ...: the layout of kmu_kfilter_export"""
    w = np.empty(2 * planes[0].size, np.uint64)
    w[0::2], w[1::2] = planes
    return w


def classes(planes, v, n_hashes):
    """0: never added; 1: added exactly once; 2: may have been added twice or more"""
    a, b = planes
    cell, mask = cell_mask(v, a.size, n_hashes)
    in_a = (a[cell] & mask) == mask
    in_b = (b[cell] & mask) == mask
    return np.where(in_a, np.where(in_b, 2, 1), 0).astype(np.uint8)


def merge(p1, p2):
    """the filter of the concatenated input"""
    return p1[0] | p2[0], p1[1] | p2[1] | (p1[0] & p2[0])


def popcount(x):
    return int(np.unpackbits(np.ascontiguousarray(x, np.uint64).view(np.uint8)).sum())


def est_distinct(n_cells, n_hashes, bits_a):
    m = 64.0 * n_cells
    if bits_a >= m:
        return math.inf
    return -(m / n_hashes) * math.log(1.0 - bits_a / m)


def cells_for(expected_distinct, bits_per_kmer):
    cells = max(1, -(-expected_distinct * bits_per_kmer // 64))
    return 0 if cells > (1 << 32) - 1 else cells

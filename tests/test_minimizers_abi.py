"""-m "not gpu": the host side of the window minimizers -- kmu_minimizer_layout (plain host C in the library), the symbols and
their bindings, the constants, the index arithmetic of minimizer.seed_hits on a stub context, and `reference_minimizers`: the
rules of include/kmu.h as plain numpy, which tests/test_gpu_minimizers.py compares the device against.  The reference is itself
checked here against a brute force over windows, on hashes drawn from tiny ranges so that ties are everywhere."""
import os
import re

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import lib, minimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def n_windows(L, k, w):
    nk = max(0, L - k + 1)
    return 0 if nk == 0 else max(nk - w, 0) + 1


def reference_minimizers(h, offsets, k, w):
    """(hashes, pos, read, mini_offsets) by the text of include/kmu.h.  h: the array of kmu_kmer_hashes (h[offsets[i] + p] is the
    hash of position p of read i); offsets: n_seq + 1 base offsets, offsets[0] may be above 0 (h is indexed from it)."""
    h = np.asarray(h, np.uint64)
    off = np.asarray(offsets).astype(np.int64)
    hashes, pos, read, moff = [], [], [], [0]
    for i in range(len(off) - 1):
        nk = max(0, int(off[i + 1] - off[i]) - k + 1)
        if nk > 0:
            hr = h[off[i] - off[0]: off[i] - off[0] + nk]
            if nk <= w:
                choice = np.array([int(np.argmin(hr))])  # (np.argmin keeps the first occurrence)
            else:
                choice = np.lib.stride_tricks.sliding_window_view(hr, w).argmin(axis=1) + np.arange(nk - w + 1)
            keep = np.ones(choice.size, bool)
            keep[1:] = choice[1:] != choice[:-1]
            p = choice[keep]
            hashes.append(hr[p])
            pos.append(p)
            read.append(np.full(p.size, i))
        moff.append(moff[-1] + (pos[-1].size if nk > 0 else 0))
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)  # noqa: E731
    return cat(hashes, np.uint64), cat(pos, np.uint32), cat(read, np.uint32), np.array(moff, np.uint64)


def brute_force_minimizers(hr, w):
    """the positions of one read's minimizers, window by window, with no library call that has a tie rule of its own"""
    nk = len(hr)
    if nk == 0:
        return []
    chosen = []
    for j in range(max(nk - w, 0) + 1):
        best = j
        for p in range(j, min(j + w, nk)):
            if hr[p] < hr[best]:  # strictly smaller: ties stay with the smallest position
                best = p
        if not chosen or chosen[-1] != best:
            assert not chosen or best > chosen[-1]  # the choice never goes back
            chosen.append(best)
    return chosen


@pytest.mark.parametrize("hi", [2, 4, 1 << 62])
def test_reference_equals_the_brute_force_under_ties(hi):
    rng = np.random.default_rng(hi % 1000)
    k = 5
    for w in (1, 2, 3, 7, 16):
        lens = [0, 1, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w, 40, 97]
        off = np.zeros(len(lens) + 1, np.int64)
        off[1:] = np.cumsum(lens)
        h = rng.integers(0, hi, size=int(off[-1]) + 1).astype(np.uint64)
        hashes, pos, read, moff = reference_minimizers(h, off, k, w)
        for i, L in enumerate(lens):
            nk = max(0, L - k + 1)
            want = brute_force_minimizers(h[off[i]: off[i] + nk].tolist(), w)
            b, e = int(moff[i]), int(moff[i + 1])
            assert pos[b:e].tolist() == want and (read[b:e] == i).all()
            assert hashes[b:e].tolist() == [int(h[off[i] + p]) for p in want]
            assert e - b <= n_windows(L, k, w)


def test_reference_poly_a_and_w1():
    h = np.zeros(50, np.uint64)
    _, pos, _, _ = reference_minimizers(h, [0, 50], 11, 8)  # nk = 40, 33 windows: every window start, nothing behind
    assert pos.tolist() == list(range(33))
    h = np.arange(30, dtype=np.uint64)[::-1].copy()
    _, pos, _, _ = reference_minimizers(h, [0, 30], 11, 1)  # w = 1: every k-mer
    assert pos.tolist() == list(range(20))


def test_layout_through_the_library():
    """fails without the feature: the symbol is missing"""
    L = lib.load()
    assert "kmu_minimizer_layout" in lib.SYMBOLS and "kmu_read_minimizers" in lib.SYMBOLS
    assert hasattr(L, "kmu_minimizer_layout") and hasattr(L, "kmu_read_minimizers")
    assert len(L.kmu_minimizer_layout.argtypes) == 5 and len(L.kmu_read_minimizers.argtypes) == 13
    k, w = 21, 10
    lens = [0, k - 1, k, k + w - 2, k + w - 1, k + w]
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    got = lib.minimizer_layout(off, k, w)
    assert got.dtype == np.uint64 and np.diff(got.astype(np.int64)).tolist() == [0, 0, 1, 1, 1, 2] and got[0] == 0
    # offsets[0] != 0: a batch inside a larger array
    got = lib.minimizer_layout(off[2:] , k, w)
    assert got.tolist() == [0, 1, 2, 3, 5]
    assert lib.minimizer_layout(off + np.uint64(1000), k, w).tolist() == lib.minimizer_layout(off, k, w).tolist()
    # w = 1: one window per k-mer; w = MAX_W is accepted
    assert np.diff(lib.minimizer_layout(off, k, 1).astype(np.int64)).tolist() == [max(0, n - k + 1) for n in lens]
    assert lib.minimizer_layout(np.array([0, 1000], np.uint64), k, A.MINIMIZER_MAX_W).tolist() == [0, 1000 - k + 1 - 256 + 1]
    for rows in range(40):  # the layout agrees with the rule the reference above is written from
        lens = np.random.default_rng(rows).integers(0, 90, size=7)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        assert np.diff(lib.minimizer_layout(off, 7, 5).astype(np.int64)).tolist() == [n_windows(int(n), 7, 5) for n in lens]


def test_layout_bad_arguments():
    L = lib.load()
    off = np.array([0, 100], np.uint64)
    out = np.zeros(2, np.uint64)
    p, q = off.ctypes.data, out.ctypes.data
    assert L.kmu_minimizer_layout(p, 1, 21, 10, q) == A.OK
    assert L.kmu_minimizer_layout(None, 1, 21, 10, q) == A.E_BAD_ARG
    assert L.kmu_minimizer_layout(p, 1, 21, 10, None) == A.E_BAD_ARG
    assert L.kmu_minimizer_layout(p, 1, 0, 10, q) == A.E_BAD_ARG
    assert L.kmu_minimizer_layout(p, 1, 21, 0, q) == A.E_BAD_ARG
    assert L.kmu_minimizer_layout(p, 1, 21, A.MINIMIZER_MAX_W + 1, q) == A.E_BAD_ARG
    with pytest.raises(lib.KmuError) as e:
        lib.minimizer_layout(off, 21, 0)
    assert e.value.code == A.E_BAD_ARG
    assert L.kmu_minimizer_layout(p, 0, 21, 10, q) == A.OK and out[0] == 0  # no read: one entry


def test_constants_match_the_header():
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    assert int(re.search(r"#define KMU_MINIMIZER_MAX_W (\d+)", txt).group(1)) == A.MINIMIZER_MAX_W == 256
    assert int(re.search(r"#define KMU_MINIMIZER_TILE (\d+)", txt).group(1)) == A.MINIMIZER_TILE
    assert "int kmu_minimizer_layout(const uint64_t *offsets" in txt and "int kmu_read_minimizers(kmu_ctx *ctx" in txt
    assert callable(getattr(lib.Context, "read_minimizers")) and lib.MINIMIZERS_WANT == ("pos", "read", "strand")


# ---- seed_hits on a stub context ------------------------------------------------------------------------------------------------
class _StubIndex:
    def __init__(self, ctx, hashes_db, n_keys, group_db):
        self.ctx = ctx
        ctx.created = (hashes_db, n_keys, group_db)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.closed = True

    def match(self, hashes_q, group_q=None, min_common=1, max_occ=0):
        self.ctx.matched = (hashes_q, group_q, min_common, max_occ)
        return self.ctx.pairs, np.zeros((self.ctx.pairs.shape[0], 3), np.uint32)


class _StubContext:
    def __init__(self, pairs):
        self.pairs = np.array(pairs, np.uint32).reshape(-1, 2)
        self.closed = False

    def anchor_index(self, hashes_db, n_keys=1, group_db=None):
        return _StubIndex(self, hashes_db, n_keys, group_db)


def _mini(hashes, pos, read, strand):
    return minimizer.Minimizers(np.array(hashes, np.uint64), np.array(pos, np.uint32), np.array(read, np.uint32),
                                None if strand is None else np.array(strand, np.uint8), None, 21, 10, A.FHASH_CANON_INVHASH)


def test_seed_hits_index_arithmetic():
    q = _mini([5, 9, 5, 7], [3, 40, 11, 70000], [0, 0, 1, 2], [0, 1, 1, 0])
    stub = _StubContext([[0, 2], [2, 0], [3, 1]])
    rec = minimizer.seed_hits(stub, q, max_occ=3)
    assert rec.dtype == np.int64 and rec.tolist() == [[0, 3, 0, 1, 11, 1], [1, 11, 1, 0, 3, 0], [2, 70000, 0, 0, 40, 1]]
    rows_db, n_keys, group_db = stub.created
    rows_q, group_q, min_common, max_occ = stub.matched
    assert rows_db.shape == (4, 1) and rows_q.shape == (4, 1) and rows_db[:, 0].tolist() == [5, 9, 5, 7]
    assert n_keys == 1 and group_db is q.read and group_q is q.read and (min_common, max_occ) == (1, 3) and stub.closed
    # a database of its own: no groups (the two batches number their reads independently); strands that were not made are 0
    db = _mini([7, 5], [8, 2], [0, 0], None)
    stub = _StubContext([[3, 0], [0, 1]])
    rec = minimizer.seed_hits(stub, q, db)
    assert rec.tolist() == [[2, 70000, 0, 0, 8, 0], [0, 3, 0, 0, 2, 0]]
    assert stub.created[2] is None and stub.matched[1] is None and stub.matched[3] == 0 and stub.created[0].shape == (2, 1)
    # no hit at all
    assert minimizer.seed_hits(_StubContext([]), q).shape == (0, 6)

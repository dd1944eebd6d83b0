"""scripts/uq_idle_waves.py counts, from read lengths alone, the wave-turns the multiset kernels' group skip still issues and the ones
that hold a k-mer.  On a handful of hand-made lengths its counts equal a brute-force walk over every thread's register slots."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts"))

import uq_idle_waves as W  # noqa: E402

UQ_KREG = 20


def _brute_uq(span, threads):
    """every slot of every thread: place 4 (tid + T g) + u of group g; a group is issued if any thread has a k-mer in it, a
    wave-turn is needed if one of the wave's 64 threads has"""
    issued = needed = 0
    for g in range(UQ_KREG // 4):
        has = [any(4 * (tid + threads * g) + u < span for u in range(4)) for tid in range(threads)]
        if any(has):
            issued += threads // 64
            needed += sum(any(has[64 * w:64 * w + 64]) for w in range(threads // 64))
    return issued, needed


def _brute_long(n_p):
    """slot q of thread t = entry 1024 q + t of the sub-list"""
    issued = needed = 0
    for g in range(UQ_KREG // 4):
        has = [any(1024 * (4 * g + u) + tid < n_p for u in range(4)) for tid in range(1024)]
        if any(has):
            issued += 16
            needed += sum(any(has[64 * w:64 * w + 64]) for w in range(16))
    return issued, needed


def test_uq_wave_turns_equal_a_brute_force_count():
    for threads, spans in ((512, (1, 255, 256, 257, 2047, 2048, 2049, 2305, 5000, 10239, 10240)),
                           (1024, (10241, 12288, 12289, 12545, 16384, 20223, 20225, 20480))):
        issued, needed = W.uq_wave_turns(np.array(spans), threads)
        for s, i, n in zip(spans, issued.tolist(), needed.tolist()):
            assert (i, n) == _brute_uq(s, threads), (threads, s)


def test_long_wave_turns_equal_a_brute_force_count():
    lens = (1, 63, 64, 65, 1023, 1024, 1025, 4096, 4097, 4160, 4161, 5119, 5120, 5121, 13333, 16384, 20480)
    issued, needed = W.long_wave_turns(np.array(lens))
    for n_p, i, n in zip(lens, issued.tolist(), needed.tolist()):
        assert (i, n) == _brute_long(n_p), n_p


def test_table_routes_reads_by_span():
    """lengths at lead 0 (each a multiple of 16 bases): one read per route; a read without a k-mer is nobody's"""
    k = 31
    lens = np.array([16, 288, 10288, 20528, 40032, 48])
    rows = W.table(lens, k)
    assert [r[1] for r in rows] == [2, 1, 2]  # (the reads of 258 and 18 k-mers; of 10 258; of 20 498 and 40 002)
    assert rows[0][2:] == (2 * 8, 2 + 1) and rows[1][2:] == (3 * 16, 41)  # (issued, needed)

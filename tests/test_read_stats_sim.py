"""The definitions of the read statistics without a GPU: the integer model (tests/read_stats_model.py) against the reference's
floating-point forms, the bucket function against its own inverse, and kmerutils_amd/statutils.py's quantile and its two dumps on
hand-written cases."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_stats_model as M  # noqa: E402


def round_half_away(x):
    """f64::round on non-negative values: x - floor(x) is exact"""
    f = np.floor(x)
    return (f + (x - f >= 0.5)).astype(np.uint64)


def test_pct_is_the_rounded_percentage_for_every_short_read():
    """((100 * h) as f64 / L as f64).round() as usize, statutils.rs:255-256, for every L <= 2000 with every h"""
    for length in range(1, 2001):
        h = np.arange(length + 1, dtype=np.uint64)
        want = round_half_away((100 * h).astype(np.float64) / np.float64(length))
        assert np.array_equal(M.pct(h, np.full(h.size, length, np.uint64)), want), length
    assert M.pct(0, 0) == 0  # (0 / 0 is NaN, and NaN as usize is 0)
    assert (M.pct(1, 8), M.pct(1, 200), M.pct(1, 40)) == (13, 1, 3)  # ties go up


def test_pct_for_long_reads():
    rng = np.random.default_rng(0x51A7)
    length = rng.integers(1, 1 << 40, 200_000, dtype=np.uint64)
    h = (rng.random(200_000) * (length + np.uint64(1)).astype(np.float64)).astype(np.uint64)
    h = np.minimum(h, length)
    want = round_half_away((100 * h).astype(np.float64) / length.astype(np.float64))
    assert np.array_equal(M.pct(h, length), want)
    assert all(M.pct(int(a), int(b)) == int(c) for a, b, c in zip(h[:2000], length[:2000], want[:2000]))


def test_quality_class_is_remap_quality8():
    """quality.rs:33-43 with its f32 expression, for all 256 bytes; the mirror's remap_quality8 is the same table"""
    from kmerutils_amd import quality
    want = np.zeros(256, np.uint8)
    for q in range(256):
        if q > 0x37:
            want[q] = 7
        elif q >= 0x25:
            nqf = np.float32(min(q, 0x37) - 0x25) * np.float32(6.0) / np.float32(18.0)
            want[q] = 1 + int(np.floor(nqf))
    assert np.array_equal(M.QUAL_CLASS, want)
    assert np.array_equal(quality.remap_quality8(np.arange(256, dtype=np.uint8)), want)
    assert [quality.remap_quality8(q) for q in (0x00, 0x24, 0x25, 0x27, 0x28, 0x36, 0x37, 0x38, 0xFF)] == [0, 0, 1, 1, 2, 6, 7, 7, 7]
    assert quality.quality_to_proba(30, 40) == 10.0 and quality.quality_to_proba(40, 40) == 1.0


def test_base_class_table():
    for c, letters in enumerate(("Aa", "Cc", "Gg", "Tt")):
        assert all(M.BASE_CLASS[ord(ch)] == c for ch in letters)
    assert int((M.BASE_CLASS == 4).sum()) == 248 and all(M.BASE_CLASS[b] == 4 for b in (ord("N"), ord("n"), 10, 0, 255))


@pytest.mark.parametrize("sig", [1, 2, 3, 4, 5])
def test_bucket_function(sig):
    """continuous and non-decreasing over 0 .. 2^21, and the range of bucket(len) brackets len"""
    lengths = np.arange((1 << 21) + 1, dtype=np.int64)
    b = M.len_buckets(lengths, sig)
    step = np.diff(b)
    assert b[0] == 0 and ((step == 0) | (step == 1)).all()
    sub = M.SUB_BITS[sig]
    assert np.array_equal(b[:1 << sub], lengths[:1 << sub])  # a bucket each below 2^sub_bits
    for length in [0, 1, (1 << sub) - 1, 1 << sub, (1 << sub) + 1, 3 << sub, (1 << 21) - 1, 1 << 21, 1 << 40, (1 << 40) + 12345]:
        bucket = M.len_bucket(length, sig)
        lo, hi = M.bucket_range(bucket, sig)
        assert lo <= length <= hi, (length, bucket, lo, hi)
        assert M.len_bucket(lo, sig) == bucket == M.len_bucket(hi, sig) and M.len_bucket(hi + 1, sig) == bucket + 1
        if length <= 1 << 21:
            assert b[length] == bucket
    first = np.flatnonzero(step == 1) + 1  # the lowest length of every bucket but the first
    for length in first[:: max(1, first.size // 500)]:
        assert M.bucket_range(int(b[length]), sig)[0] == length


def test_layout():
    assert M.layout(1_000_000, 3) == (11_264, 1_048_576)
    # sig_digits 1: 32 single buckets, ranges of 16
    assert M.layout(31, 1) == (32, 32)
    assert M.layout(32, 1) == (48, 64)
    assert M.layout(63, 1) == (48, 64)
    assert M.layout(64, 1) == (64, 128)
    for max_len, sig in ((1_000_000, 3), (31, 1), (32, 1), (63, 1), (5000, 3), (1, 5)):
        n_buckets, limit = M.layout(max_len, sig)
        assert limit > max_len >= limit // 2 or limit == 1 << M.SUB_BITS[sig]
        assert M.len_bucket(limit - 1, sig) == n_buckets - 1  # the last bucket ends where the histogram does


# ---- kmerutils_amd/statutils.py: the quantile and the dumps (they need the library's two layout calls, no device) ----
@pytest.fixture(scope="module")
def statutils():
    from kmerutils_amd import build, statutils
    build.build()
    return statutils


def distribution(statutils, lengths, pct_hist=None, prec=3, max_len=1_000_000):
    n_buckets, limit = M.layout(max_len, prec)
    lengths = np.asarray(lengths, np.int64)
    inside = lengths[lengths < limit]
    len_hist = np.bincount(M.len_buckets(inside, prec), minlength=n_buckets).astype(np.uint64)
    pct_hist = np.zeros((101, 4), np.uint64) if pct_hist is None else pct_hist
    return statutils.ReadBaseDistribution(pct_hist, len_hist, lengths.size, lengths.size - inside.size, 0, max_len, prec)


def test_number_format(statutils):
    got = [statutils.rust_display(x) for x in (0.0, 1.0, 0.5, 1 / 3, 1 / 3e6, 100.0, 2.5e-5)]
    assert got == ["0", "1", "0.5", "0.3333333333333333", "0.00000033333333333333335", "100", "0.000025"]


def test_value_at_quantile(statutils):
    d = distribution(statutils, [5, 5, 5, 3000])  # 3000 shares its bucket with 3001
    assert [d.value_at_quantile(q) for q in (0.0, 0.5, 0.75, 0.76, 1.0)] == [5, 5, 5, 3001, 3001]
    assert distribution(statutils, []).value_at_quantile(0.5) == 0
    d = distribution(statutils, [10, 2_000_000])  # the second read is beyond the histogram
    assert d.histo_out == 1 and d.readsize_len() == 1 and d.value_at_quantile(1.0) == 10


def test_readlen_dump_hand_case(statutils, tmp_path):
    """1000 reads of the lengths 1 .. 1000: nb_entries = maxlen = 1000, nbslot = 10, readsize = [1, 100, 200, .. 1000]; threshold j
    passes readsize[i] at j = 100 i + 1, where slot i + 1 is reported with 100 reads -- except the last, which `current_i < nbslot`
    leaves out (statutils.rs:163)"""
    d = distribution(statutils, np.arange(1, 1001))
    name = tmp_path / "readlen.histo"
    assert d.ascii_dump_readlen_distribution(str(name)) is None
    assert name.read_text() == "".join("%d  100 \n" % (100 * i) for i in range(1, 10))
    # 200 reads: two slots, one line
    d = distribution(statutils, np.arange(1, 201))
    assert d.ascii_dump_readlen_distribution(str(name)) is None
    assert name.read_text() == "100  100 \n"


def test_readlen_dump_refuses_fewer_than_100_entries(statutils, tmp_path):
    name = tmp_path / "readlen.histo"
    for lengths in ([], np.arange(1, 100)):
        err = distribution(statutils, lengths).ascii_dump_readlen_distribution(str(name))
        assert isinstance(err, OSError) and "histogram error!" in str(err) and not name.exists()


def test_acgt_dump_hand_case(statutils, tmp_path):
    pct_hist = np.zeros((101, 4), np.uint64)
    pct_hist[0] = [3, 0, 1, 2]
    pct_hist[50] = [0, 3, 0, 0]
    pct_hist[100] = [0, 0, 2, 1]
    d = distribution(statutils, [10, 20, 30], pct_hist)
    name = tmp_path / "bases.histo"
    d.ascii_dump_acgt_distribution(str(name))
    lines = name.read_text().split("\n")
    assert len(lines) == 102 and lines[101] == ""
    assert lines[0] == "1 0  0.3333333333333333  0.6666666666666666 "
    assert lines[50] == "0 1  0  0 "
    assert lines[100] == "0 0  0.6666666666666666  0.3333333333333333 "
    assert all(line == "0 0  0  0 " for i, line in enumerate(lines[:101]) if i not in (0, 50, 100))

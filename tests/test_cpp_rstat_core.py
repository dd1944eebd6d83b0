"""kmu_rstat_core.h -- the arithmetic the kernels of kmu_read_stats.hip are written on -- compiled for the host: the stand-alone
program tests/cpp/rstat_core_check.cpp (its own main, no GPU, no libkmu) is built with AddressSanitizer and
UndefinedBehaviorSanitizer (the fixture prints which build ran: a g++ that cannot link their runtimes builds it plain), runs as a
child process, and every value it prints is compared with the numpy model."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import read_stats_model as M  # noqa: E402

SOURCE = os.path.join(HERE, "cpp", "rstat_core_check.cpp")
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rstat_core")
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp / "probe")], capture_output=True).returncode == 0
    exe = tmp / "rstat_core_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra"] + (SAN if linked else ["-O1"]) + [SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("rstat_core_check: sanitizer runtimes", "linked" if linked else "absent, plain build")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = {}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        got.setdefault(word, []).append([int(v) for v in rest.split()])
    return got


def test_classes(printed):
    assert printed["base"] == [M.BASE_CLASS.tolist()]
    assert printed["qual"] == [M.QUAL_CLASS.tolist()]
    assert printed["sub_bits"] == [[s, M.SUB_BITS.get(s, 0)] for s in range(7)]


def test_pct(printed):
    assert len(printed["pct"]) == 2001
    for row in printed["pct"]:
        length = row[0]
        h = np.arange(length + 1, dtype=np.uint64)
        assert row[1:] == M.pct(h, np.full(h.size, length, np.uint64)).tolist(), length
    assert printed["pct_long"] == [[M.pct((1 << 40) // 3, 1 << 40), 100]]


def test_buckets_and_layout(printed):
    assert len(printed["bucket"]) == 5 * (4201 + 51 * 3)
    for sig, length, bucket, lo, hi in printed["bucket"]:
        assert bucket == M.len_bucket(length, sig) and (lo, hi) == M.bucket_range(bucket, sig), (sig, length)
    lengths = np.arange((1 << 21) + 1, dtype=np.int64)
    assert printed["bucketsum"] == [[sig, int(M.len_buckets(lengths, sig).sum())] for sig in range(1, 6)]
    assert len(printed["layout"]) == 40
    for max_len, sig, n_buckets, limit in printed["layout"]:
        assert (n_buckets, limit) == M.layout(max_len, sig), (max_len, sig)


def test_median_class(printed):
    rows = [[0] * 8, [1, 0, 0, 0, 0, 0, 0, 0], [2, 0, 0, 2, 0, 0, 0, 0], [1, 0, 0, 2, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 9], [3, 1, 1, 1, 1, 1, 1, 2]]
    assert printed["median"] == [[M.median_class(r, sum(r))] for r in rows]
    assert [m for (m,) in printed["median"]] == [0, 0, 0, 3, 7, 3]

"""The C++ mirror of the read statistics (include/kmerutils.hpp: ReadBaseDistribution, get_base_count_par, ingest_fastq_qual,
read_quality_stats) through its own test program, tests/cpp/test_read_stats.cpp, run as a child process: the hand cases inside the
program, and a FASTQ text handed over in a file, whose statistics and dumps this test compares with the numpy model."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_read_stats  # noqa: E402  (tests/cpp/build_read_stats.py)
import read_stats_model as M  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_read_stats.build()


def test_read_stats_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_read_stats" in r.stdout and "no CPU fallback" in r.stdout


def fastq_text(n_reads, seed):
    """reads of 1 .. 3000 bases with qualities over the whole class range, some records with N, some CRLF, no final newline"""
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(n_reads):
        length = int(rng.integers(1, 3000)) if i % 7 else int(rng.integers(1, 40))
        seq = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), length, p=[.3, .2, .2, .2, .025, .025, .025, .025])
        if i % 11 == 5:
            seq[int(rng.integers(0, length))] = ord("N")
        qual = rng.integers(0x21, 0x4B, length).astype(np.uint8)
        end = b"\r\n" if i % 5 == 2 else b"\n"
        recs.append(b"@r%d" % i + end + seq.tobytes() + end + b"+" + end + qual.tobytes() + end)
    text = b"".join(recs)
    return text[:-1] if text.endswith(b"\n") and not text.endswith(b"\r\n") else text


@pytest.mark.gpu
def test_file_statistics_equal_the_model(test_bin, tmp_path):
    from kmerutils_amd import statutils
    text = fastq_text(240, 0xC0FFEE)
    (tmp_path / "reads.fastq").write_bytes(text)
    r = subprocess.run([test_bin, str(tmp_path / "reads.fastq"), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_read_stats" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"kept": [], "read": [], "totals": [], "len": [], "readlen_error": [], "qual": [], "classes": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(rest.split())
    bases, quals, off, _ = M.ingest_fastq_qual(text)
    n = off.size - 1
    assert got["kept"] == [[str(n), str(bases.size)]] and n < 240
    assert [(int(a), bytes.fromhex(b)) for a, b in got["read"]] == [
        (int(off[i + 1] - off[i]), quals[int(off[i]):int(off[i + 1])].tobytes()) for i in range(n)]
    _, pct_hist, len_hist, info = M.read_stats(bases, off)
    assert got["totals"] == [[str(n), "0", "0"]]
    assert [(int(b), int(c)) for b, c in got["len"]] == [(int(b), int(len_hist[b])) for b in np.flatnonzero(len_hist)]
    want = statutils.ReadBaseDistribution(pct_hist, len_hist, n, info["histo_out"], info["n_other"], 1_000_000, 3)
    want.ascii_dump_acgt_distribution(str(tmp_path / "want_bases.histo"))
    assert want.ascii_dump_readlen_distribution(str(tmp_path / "want_readlen.histo")) is None and got["readlen_error"] == [["0"]]
    assert (tmp_path / "bases.histo").read_bytes() == (tmp_path / "want_bases.histo").read_bytes()
    assert (tmp_path / "readlen.histo").read_bytes() == (tmp_path / "want_readlen.histo").read_bytes()
    recs, hist = M.read_qual_stats(quals, off)
    assert [[int(v) for v in row] for row in got["qual"]] == [
        [int(v) for v in recs["n_class"][i]] + [int(recs["sum_q"][i]), int(recs["min_q"][i]), int(recs["max_q"][i]), int(recs["median_class"][i])]
        for i in range(n)]
    assert [[int(v) for v in row] for row in got["classes"]] == [[int(v) for v in hist]]

"""The C++ mirror of the syncmers (include/kmerutils.hpp: read_syncmers) through its own test program,
tests/cpp/test_syncmers.cpp, run as a child process: reads at the tile edges against a plain loop over the mirror's own kmer_hashes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_syncmers  # noqa: E402  (tests/cpp/build_syncmers.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_syncmers.build()


def test_syncmers_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        return  # (with a device the program runs: the test below)
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_read_syncmers" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_read_syncmers_against_the_plain_loop(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_read_syncmers" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

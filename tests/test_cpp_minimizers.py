"""The C++ mirror of the window minimizers (include/kmerutils.hpp: minimizer_layout, read_minimizers) through its own test
program, tests/cpp/test_minimizers.cpp, run as a child process: reads against a plain loop over the mirror's own kmer_hashes."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_minimizers  # noqa: E402  (tests/cpp/build_minimizers.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_minimizers.build()


def test_minimizers_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_read_minimizers" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_read_minimizers_against_the_plain_loop(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_read_minimizers" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

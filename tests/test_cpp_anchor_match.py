"""The C++ mirror of the anchor matching (include/kmerutils.hpp: match_read_anchors) through its own test program,
tests/cpp/test_anchor_match.cpp, run as a child process: a read and its first half among unrelated reads, against a brute force
written in the program."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_anchor_match  # noqa: E402  (tests/cpp/build_anchor_match.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_anchor_match.build()


def test_anchor_match_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_match_read_anchors" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_match_read_anchors_against_the_brute_force(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_match_read_anchors" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

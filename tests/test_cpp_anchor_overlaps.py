"""The C++ mirror of the read overlaps (include/kmerutils.hpp: anchor_overlaps, read_overlaps) through its own test program,
tests/cpp/test_anchor_overlaps.cpp, run as a child process: reads cut from one genome, one of them reverse-complemented, against
a vote over the hits of match_read_anchors written in the program."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_anchor_overlaps  # noqa: E402  (tests/cpp/build_anchor_overlaps.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_anchor_overlaps.build()


def test_anchor_overlaps_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_anchor_overlaps" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_read_overlaps_against_the_vote_in_the_program(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_anchor_overlaps" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

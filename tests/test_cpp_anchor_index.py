"""The C++ mirror of the anchor index (include/kmerutils.hpp: AnchorIndex, and max_occ of match_read_anchors / read_overlaps)
through its own test program, tests/cpp/test_anchor_index.cpp, run as a child process: rows with one hash that a third of the
database carries, with and without a repeat mask, against a brute force written in the program."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_anchor_index  # noqa: E402  (tests/cpp/build_anchor_index.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_anchor_index.build()


def test_anchor_index_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_anchor_index" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_anchor_index_against_the_brute_force(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok test_anchor_index" in r.stdout and "ok test_match_read_anchors_with_a_mask" in r.stdout

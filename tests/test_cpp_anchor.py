"""The C++ mirror of the read anchors (include/kmerutils.hpp: gen_read_anchors) through its own test program,
tests/cpp/test_anchor.cpp, run as a child process: three reads against the oracle's rows of the substrings."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_anchor  # noqa: E402  (tests/cpp/build_anchor.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_anchor.build()


def test_anchor_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_gen_read_anchors" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_gen_read_anchors_against_the_oracle(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_gen_read_anchors" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

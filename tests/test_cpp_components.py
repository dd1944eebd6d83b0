"""The C++ mirror of the connected components (include/kmerutils.hpp: components, components_knn, read_clusters) through its own
test program, tests/cpp/test_components.cpp, run as a child process: hand cases, one long path and the clusters of reads cut from
three genomes, against a union-find written in the program."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_components  # noqa: E402  (tests/cpp/build_components.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_components.build()


def test_components_program_builds_and_refuses_to_run_without_a_device(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "FAIL test_components" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_components_against_the_union_find_in_the_program(test_bin):
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_components" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]

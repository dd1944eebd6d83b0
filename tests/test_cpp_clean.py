"""The C++ mirror of string graph cleaning (include/kmerutils.hpp: sg_clean, clean_graph, layout_reads) through its own test
program, tests/cpp/test_clean.cpp, run as a child process: the hand case inside the program, and two planted cases of
tests/test_clean_abi.py, whose arcs this test hands over in a file and whose cleaned arcs, summaries and counts, as the program
prints them, it compares with the arrays of the Python reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_clean  # noqa: E402  (tests/cpp/build_clean.py)
from test_clean_abi import STATS, cleaned_case, planted_case, reference_clean, removed_reads  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_clean.build()


def test_clean_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_clean" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("name,T,B", [("mix", 4, 8), ("bubbles", 64, 64)])
def test_cleaning_equals_the_reference(test_bin, tmp_path, name, T, B):
    arcs, n_reads, _ = planted_case(name)
    rows = ["%d %d %d" % (n_reads, T, B)] + [" ".join(str(v) for v in x[:7]) for x in arcs.tolist()]
    (tmp_path / "arcs.txt").write_text("\n".join(rows) + "\n")
    r = subprocess.run([test_bin, str(tmp_path / "arcs.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_clean" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"arc": [], "read": [], "stats": [], "rounds": [], "unitigs": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(tuple(int(v) for v in rest.split()))
    want = cleaned_case(name, T, B)
    assert got["arc"] == [tuple(x) for x in want[0].tolist()] and got["read"] == [tuple(x) for x in want[1].tolist()]
    assert got["stats"] == [tuple(want[2][k] for k in STATS)]
    again = reference_clean(want[0], n_reads, T, B, want[1])
    assert got["rounds"] == [tuple(again[2][k] if k == "n_arcs_left" else want[2][k] + again[2][k] for k in STATS)]
    assert got["unitigs"][0][1] == n_reads - len(removed_reads(want[1]))

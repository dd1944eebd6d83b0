"""The C++ mirror of the string graph (include/kmerutils.hpp: sg_classify, overlap_graph, unitig_labels, gfa_line) through its own
test program, tests/cpp/test_string_graph.cpp, run as a child process: the hand cases inside the program, and planted layout (i)
with strands and read numbers of the program's choice, whose chain records and arcs the program prints and this test compares with
the Python route and with the reference on the same records."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_string_graph  # noqa: E402  (tests/cpp/build_string_graph.py)
from test_string_graph_abi import offsets_of, params, records, reference_graph  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_string_graph.build()


def test_string_graph_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_string_graph" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_arcs_equal_the_python_route_and_the_reference(test_bin):
    from kmerutils_amd import lib
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_string_graph" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"chain": [], "arc": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(tuple(int(v) for v in rest.split()))
    assert len(got["chain"]) == 75 and len(got["arc"]) == 150
    chains, offsets, p = records(got["chain"]), offsets_of([400] * 27), params()
    ctx = lib.Context(0)
    try:
        arcs = ctx.sg_graph(chains, None, offsets, **p)[0]
    finally:
        ctx.close()
    assert [tuple(x)[:7] for x in arcs.tolist()] == got["arc"]
    assert arcs.tobytes() == reference_graph(chains, None, offsets, **p)[0].tobytes()

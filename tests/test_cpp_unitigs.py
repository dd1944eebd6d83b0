"""The C++ mirror of the unitig layout (include/kmerutils.hpp: sg_unitigs, unitig_sequences, unitig_gfa_line) through its own test
program, tests/cpp/test_unitigs.cpp, run as a child process: the hand cases inside the program, and planted layout (i), whose
chain records this test hands over in a file and whose unitigs, steps and places, as the program prints them, it compares with
the Python route and with the reference."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_unitigs  # noqa: E402  (tests/cpp/build_unitigs.py)
from test_string_graph_abi import planted_tiling  # noqa: E402
from test_unitigs_abi import planted_unitigs  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_unitigs.build()


def test_unitigs_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_unitigs" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_unitigs_equal_the_python_route_and_the_reference(test_bin, tmp_path):
    from kmerutils_amd import lib, minimizer
    chains, offsets, _, p = planted_tiling(0)
    lengths = np.diff(offsets.astype(np.int64))
    rows = ["%d" % len(lengths), " ".join(str(int(x)) for x in lengths)]
    rows += ["%d %d %d %d %d %d %d" % (c["read_a"], c["read_b"], c["strand"], c["a_start"], c["a_end"], c["b_start"], c["b_end"]) for c in chains]
    (tmp_path / "records.txt").write_text("\n".join(rows) + "\n")
    r = subprocess.run([test_bin, str(tmp_path / "records.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_unitigs" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"unitig": [], "step": [], "place": [], "bytes": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(tuple(int(v) for v in rest.split()))
    ctx = lib.Context(0)
    try:
        arcs, _, _, reads = minimizer.overlap_graph(ctx, chains, None, offsets, **p)
        unitigs, path, place = minimizer.unitig_paths(ctx, arcs, reads, offsets)
    finally:
        ctx.close()
    assert [tuple(x)[:5] for x in unitigs.tolist()] == got["unitig"] and len(got["unitig"]) == 1
    assert [tuple(x) for x in path.tolist()] == got["step"] and len(got["step"]) == 27
    assert [tuple(x)[:3] for x in place.tolist()] == got["place"] and got["bytes"] == [(3000,)]
    want = planted_unitigs("tiling", 0)[1]
    assert unitigs.tobytes() == want[0].tobytes() and path.tobytes() == want[1].tobytes() and place.tobytes() == want[2].tobytes()

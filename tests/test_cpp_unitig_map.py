"""The C++ mirror of the unitig map and the unitig consensus (include/kmerutils.hpp: sg_unitig_chains, unitig_read_chains,
polish_unitigs) through its own test program, tests/cpp/test_unitig_map.cpp, run as a child process: the hand case inside the
program, and the noisy planted genome of tests/test_unitig_map_abi.py, which this test hands over in a file and whose records, counts
and polished unitigs, as the program prints them, it compares with the Python reference and the Python route."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_unitig_map  # noqa: E402  (tests/cpp/build_unitig_map.py)
from test_unitig_map_abi import STATS, planted_genome, reference_unitig_chains  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_unitig_map.build()


def test_unitig_map_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_unitig_map" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("circular,rounds", [(False, 1), (True, 2)])
def test_map_and_polish_equal_the_python_route(test_bin, tmp_path, circular, rounds):
    from kmerutils_amd import lib, minimizer
    g = planted_genome(11, circular, rate=0.05, ends=0 if circular else 8)
    layout = (g["unitigs"], g["path"], g["place"])
    off = g["offsets"].astype(int)
    rows = ["%d %d %d %d %d" % (len(layout[0]), len(layout[1]), len(layout[2]), len(g["chains"]), rounds)]
    for table in layout:
        rows += [" ".join(str(v) for v in x) for x in table.tolist()]
    rows += [" ".join(str(v) for v in x) + " %d" % c for x, c in zip(g["chains"].tolist(), g["classes"].tolist())]
    rows += [g["bases"][off[r]:off[r + 1]].tobytes().decode() for r in range(len(off) - 1)]
    (tmp_path / "case.txt").write_text("\n".join(rows) + "\n")
    r = subprocess.run([test_bin, str(tmp_path / "case.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_unitig_map" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"rec": [], "stats": [], "cons": [], "step": [], "len": [], "aln": [], "used": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(rest if word == "cons" else tuple(int(v) for v in rest.split()))
    want, stats = reference_unitig_chains(*layout, g["chains"], g["classes"], g["offsets"])
    assert got["rec"] == [tuple(x) for x in want.tolist()] and got["stats"] == [tuple(stats[k] for k in STATS)]
    ctx = lib.Context(0)
    try:
        seq, seq_off = ctx.sg_unitig_seqs(g["unitigs"], g["path"], g["bases"], g["offsets"])
        cons, cons_off, new_path, _, used, aln = minimizer.polish_unitigs(ctx, *layout, seq, seq_off, g["bases"], g["offsets"], g["chains"],
                                                                          g["classes"], rounds=rounds)
    finally:
        ctx.close()
    assert got["cons"] == [cons.tobytes().decode()] and got["len"] == [(len(cons),)]
    assert got["step"] == [tuple(x) for x in new_path.tolist()] and got["aln"] == [tuple(x) for x in aln.tolist()]
    assert got["used"] == [tuple(x) for x in used[["read_b", "a_start", "a_end"]].tolist()]

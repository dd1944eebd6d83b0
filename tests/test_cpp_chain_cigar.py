"""The C++ mirror of chain alignment paths (include/kmerutils.hpp: chain_cigar, cigar_chains, cigar_string, paf_line with cg:Z:)
through its own test program, tests/cpp/test_chain_cigar.cpp, run as a child process: hand-made chains inside the program, and a
small batch of related reads whose records, runs and PAF lines the program prints and this test compares with the Python route on
the same reads and chains."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_chain_cigar  # noqa: E402  (tests/cpp/build_chain_cigar.py)
from test_chain_align_abi import chain_recs  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_chain_cigar.build()


def test_chain_cigar_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_chain_cigar" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_runs_and_paf_lines_equal_the_python_route(test_bin):
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_chain_cigar" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    reads, rows, recs, runs, paf = [], [], [], [], []
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "read":
            reads.append(rest.encode())
        elif word == "chain":
            rows.append(tuple(int(v) for v in rest.split()))
        elif word == "aln":
            recs.append(tuple(int(v) for v in rest.split()))
        elif word == "ops":
            runs.append([int(v) for v in rest.split()])
        elif word == "paf":
            paf.append(rest)
    assert len(reads) == 12 and len(rows) == len(recs) == len(runs) == len(paf) == 6
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    chains = chain_recs(rows)
    chains["score"], chains["n_seeds"], chains["n_anchors"] = 30, 2, 2
    ctx = lib.Context(0)
    try:
        aln, ops, op_off = minimizer.cigar_chains(ctx, chains, bases, off, band=16)
    finally:
        ctx.close()
    assert aln.dtype == np.dtype(A.CHAIN_ALN_DTYPE) and aln.tolist() == recs
    assert [ops[int(op_off[c]):int(op_off[c + 1])].tolist() for c in range(6)] == runs
    assert minimizer.paf_lines(chains, aln, ["q%d" % i for i in range(12)], off, cigar=(ops, op_off)) == paf

"""The C++ mirror of chain alignment (include/kmerutils.hpp: chain_align, align_chains, read_alignments, paf_line) through its own
test program, tests/cpp/test_chain_align.cpp, run as a child process: hand-made chains inside the program, and two reads of one
sequence whose alignment records and PAF lines the program prints and this test compares with the Python route on the same reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_chain_align  # noqa: E402  (tests/cpp/build_chain_align.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_chain_align.build()


def test_chain_align_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_chain_align" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_records_and_paf_lines_equal_the_python_route(test_bin):
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_chain_align" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cases, reads, recs, paf = [], [], [], []
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "read":
            reads.append(rest.encode())
        elif word == "aln":
            recs.append(tuple(int(v) for v in rest.split()))
        elif word == "paf":
            paf.append(rest)
        elif word == "end":
            cases.append((reads, recs, paf))
            reads, recs, paf = [], [], []
    assert len(cases) == 2
    ctx = lib.Context(0)
    try:
        for strand, (reads, recs, paf) in enumerate(cases):
            bases = np.frombuffer(b"".join(reads), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
            chains, aln = minimizer.read_alignments(ctx, bases, off, 15, 10, band=32)
            assert chains.shape == (1,) and chains["strand"][0] == strand
            assert aln.dtype == np.dtype(A.CHAIN_ALN_DTYPE) and aln.tolist() == recs
            assert minimizer.paf_lines(chains, aln, ["a", "b", "c"], off) == paf
    finally:
        ctx.close()

"""The C++ mirror of seed chaining (include/kmerutils.hpp: seed_chains, seed_pairs, chain_hits, read_chains) through its own test
program, tests/cpp/test_chains.cpp, run as a child process: a hand-made case inside the program, and two reads of one sequence
whose records the program prints and this test compares with the Python route on the same reads."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_chains  # noqa: E402  (tests/cpp/build_chains.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_chains.build()


def test_chains_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_chains" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_records_equal_the_python_route(test_bin):
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_chains" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    cases, reads, recs = [], [], {"chain": [], "both": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "read":
            reads.append(rest.encode())
        elif word in recs:
            recs[word].append(tuple(int(v) for v in rest.split()))
        elif word == "end":
            cases.append((reads, recs))
            reads, recs = [], {"chain": [], "both": []}
    assert len(cases) == 2
    ctx = lib.Context(0)
    try:
        for strand, (reads, recs) in enumerate(cases):
            bases = np.frombuffer(b"".join(reads), np.uint8)
            off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
            want = minimizer.read_chains(ctx, bases, off, 15, 10)
            assert want.shape == (1,) and want["strand"][0] == strand and want.tolist() == recs["chain"]
            m = minimizer.read_minimizers(ctx, bases, off, 15, 10)
            both = minimizer.chain_hits(ctx, m, m, min_seeds=1)
            assert both.dtype == np.dtype(A.CHAIN_DTYPE) and both.tolist() == recs["both"]
    finally:
        ctx.close()

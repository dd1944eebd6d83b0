"""The C++ mirror of the read pileup (include/kmerutils.hpp: chain_pileup, pileup_chains, pile_call) through its own test program,
tests/cpp/test_chain_pileup.cpp, run as a child process: hand-made chains inside the program, and a small batch of related reads
whose table rows, calls and read summaries the program prints and this test compares with the Python route on the same reads and
chains."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_chain_pileup  # noqa: E402  (tests/cpp/build_chain_pileup.py)
from test_chain_align_abi import chain_recs  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_chain_pileup.build()


def test_chain_pileup_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_chain_pileup" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_rows_calls_and_summaries_equal_the_python_route(test_bin):
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_chain_pileup" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    reads, rows, table, calls, piles = [], [], [], [], []
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "read":
            reads.append(rest.encode())
        elif word == "chain":
            rows.append(tuple(int(v) for v in rest.split()))
        elif word == "row":
            counts, _, call = rest.partition(" call ")
            table.append([int(v) for v in counts.split()])
            calls.append(int(call))
        elif word == "pile":
            piles.append(tuple(int(v) for v in rest.split()))
    assert len(reads) == 12 and len(rows) == 11 and len(piles) == 12
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    chains = chain_recs(rows)
    ctx = lib.Context(0)
    try:
        aln, ops, op_off = minimizer.cigar_chains(ctx, chains, bases, off, band=16)
        pile, _ = minimizer.pileup_chains(ctx, chains, aln, ops, op_off, bases, off)
        call, summary = ctx.pile_call(pile, bases, off, min_depth=1)
    finally:
        ctx.close()
    assert pile.tolist() == table and call.tolist() == calls and summary.tolist() == piles
    assert minimizer.pile_depth(pile).sum() == sum(p[6] for p in piles) > 0

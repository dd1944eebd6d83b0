"""The C++ mirror of read correction (include/kmerutils.hpp: pile_ins_plan, chain_pile_ins, pile_consensus, correct_chains) through
its own test program, tests/cpp/test_pile_consensus.cpp, run as a child process: a hand-made case inside the program, and a small
batch of related reads whose slot counts, slot table and corrected reads the program prints and this test compares with the Python
route on the same reads and chains."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_pile_consensus  # noqa: E402  (tests/cpp/build_pile_consensus.py)
from test_chain_align_abi import chain_recs  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_pile_consensus.build()


def test_pile_consensus_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_pile_consensus" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_slots_and_corrected_reads_equal_the_python_route(test_bin):
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_pile_consensus" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    reads, rows, slots, cons, lens = [], [], [], [], None
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word == "read":
            reads.append(rest.encode())
        elif word == "chain":
            rows.append(tuple(int(v) for v in rest.split()))
        elif word == "len":
            lens = [int(v) for v in rest.split()]
        elif word == "slot":
            slots.append([int(v) for v in rest.split()])
        elif word == "cons":
            cons.append(rest.encode())
    assert len(reads) == 8 and len(rows) == 28 and len(cons) == 8
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    chains = chain_recs(rows)
    ctx = lib.Context(0)
    try:
        aln, ops, op_off = minimizer.cigar_chains(ctx, chains, bases, off, band=16)
        pile, _ = minimizer.pileup_chains(ctx, chains, aln, ops, op_off, bases, off)
        call, _ = ctx.pile_call(pile, bases, off, min_depth=3)
        ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=4)
        ins, _ = minimizer.insertions_chains(ctx, chains, aln, ops, op_off, bases, off, ins_len, n_slots)
        cons_bases, cons_off = minimizer.consensus_reads(ctx, pile, call, ins_len, n_slots, ins, bases, off)
    finally:
        ctx.close()
    assert ins_len.tolist() == lens and n_slots == len(slots) > 0 and ins.tolist() == slots
    assert [cons_bases[int(cons_off[k]):int(cons_off[k + 1])].tobytes() for k in range(8)] == cons
    assert cons != reads

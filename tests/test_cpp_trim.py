"""The C++ mirror of read trimming (include/kmerutils.hpp: pile_segments, extract_ranges, pile_consensus_pos, trim_reads,
correct_trim_chains) through its own test program, tests/cpp/test_trim.cpp, run as a child process: the hand cases inside the
program, and a small batch with a planted chimera and a tailed read whose segments, trimmed reads and corrected reads the program
prints and this test compares with the Python route on the same reads and chains."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_trim  # noqa: E402  (tests/cpp/build_trim.py)
from test_chain_align_abi import chain_recs  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_trim.build()


def test_trim_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_trim" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_segments_and_trimmed_reads_equal_the_python_route(test_bin):
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_trim" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"read": [], "chain": [], "seg": [], "trim": [], "out": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(rest)
    reads = [x.encode() for x in got["read"]]
    assert len(reads) == 10 and len(got["chain"]) == 24 and len(got["seg"]) == len(got["trim"]) == len(got["out"]) == 11
    bases = np.frombuffer(b"".join(reads), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(x) for x in reads])]).astype(np.uint64)
    chains = chain_recs([tuple(int(v) for v in x.split()) for x in got["chain"]])
    ctx = lib.Context(0)
    try:
        aln, ops, op_off = minimizer.cigar_chains(ctx, chains, bases, off, band=8)
        pile, _ = minimizer.pileup_chains(ctx, chains, aln, ops, op_off, bases, off)
        trim, trim_off, segs, summary = minimizer.trim_reads(ctx, pile, bases, off, min_depth=3, min_span=3, min_len=20)
        call, _ = ctx.pile_call(pile, bases, off, min_depth=3)
        ins_len, n_slots = ctx.pile_ins_plan(pile, call, max_ins=16)
        ins, _ = minimizer.insertions_chains(ctx, chains, aln, ops, op_off, bases, off, ins_len, n_slots)
        cons, _ = minimizer.consensus_reads(ctx, pile, call, ins_len, n_slots, ins, bases, off)
        beg = off[segs["read"]]
        pos = ctx.pile_consensus_pos(pile, call, ins_len, n_slots, ins, bases, off, np.concatenate([beg + segs["start"], beg + segs["end"]]))
        out, out_off = ctx.extract_ranges(cons, pos[:len(segs)], pos[len(segs):])
    finally:
        ctx.close()
    assert [" ".join(str(int(v)) for v in s) for s in segs.tolist()] == got["seg"]
    assert [trim[int(trim_off[k]):int(trim_off[k + 1])].tobytes().decode() for k in range(11)] == got["trim"]
    assert [out[int(out_off[k]):int(out_off[k + 1])].tobytes().decode() for k in range(11)] == got["out"]
    assert summary["cls"].tolist() == [A.TRIM_WHOLE] * 8 + [A.TRIM_SPLIT, A.TRIM_ENDS]

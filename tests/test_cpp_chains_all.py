"""The C++ mirror of kmu_seed_chains_all and kmu_chain_rank (include/kmerutils.hpp: seed_chains_all, chain_rank, chain_mapq,
chain_hits with `all`, paf_line with a rank record) through its own test program, tests/cpp/test_chains_all.cpp, run as a child
process: a hand-made case inside the program, and a read made of two far-apart pieces of a contig whose records, ranks and mapping
qualities the program prints and this test compares with the Python route on the same sequences."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_chains_all  # noqa: E402  (tests/cpp/build_chains_all.py)


@pytest.fixture(scope="module")
def test_bin():
    return build_chains_all.build()


def test_chains_all_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_chains_all" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
def test_records_equal_the_python_route(test_bin):
    from kmerutils_amd import _abi as A
    from kmerutils_amd import lib, minimizer
    r = subprocess.run([test_bin], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_chains_all" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    seqs, recs = {}, {"all": [], "rank": [], "mapq": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in ("read", "contig"):
            seqs[word] = np.frombuffer(rest.encode(), np.uint8)
        elif word in recs:
            recs[word].append(tuple(int(v) for v in rest.split()))
    assert len(recs["all"]) == 2 and "end" in r.stdout.splitlines()
    ctx = lib.Context(0)
    try:
        off = lambda x: np.array([0, x.size], np.uint64)  # noqa: E731
        chains, rank = minimizer.map_reads(ctx, seqs["read"], off(seqs["read"]), seqs["contig"], off(seqs["contig"]), 15, 10)
        assert chains.dtype == np.dtype(A.CHAIN_DTYPE) and chains.tolist() == recs["all"]
        assert rank.dtype == np.dtype(A.CHAIN_RANK_DTYPE) and rank.tolist() == recs["rank"]
        assert [(m,) for m in minimizer.chain_mapq(chains, rank).tolist()] == recs["mapq"]
    finally:
        ctx.close()

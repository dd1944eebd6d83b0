"""The C++ mirror of the count prefilter (include/kmerutils.hpp: KmerPrefilter, count_repeated_kmers) through its own test program,
tests/cpp/test_kfilter.cpp, run as a child process: the hand case inside the program, and reads handed over in a file, whose
filter words, classes and dump entries, as the program prints them, this test compares with the numpy model and the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_kfilter  # noqa: E402  (tests/cpp/build_kfilter.py)
import kfilter_model as M  # noqa: E402


@pytest.fixture(scope="module")
def test_bin():
    return build_kfilter.build()


def test_kfilter_program_builds_and_has_no_host_fallback(test_bin):
    import torch
    assert os.access(test_bin, os.X_OK)
    if not torch.cuda.is_available():  # nothing is computed on the host: the program stops with the library's error
        r = subprocess.run([test_bin], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "FAIL test_kfilter" in r.stdout and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("ktype,k,bits,hashes", [(A.KMER64BIT, 31, 16, 4), (A.KMER16B32BIT, 16, 8, 3)], ids=["k31", "k16"])
def test_count_repeated_kmers_equals_the_model(test_bin, oracle, tmp_path, ktype, k, bits, hashes):
    b, o = synth.genome_reads(60, np.full(60, 200, np.int64), 5_000, 0xA1, sub=0.01)
    seqs = [b[int(o[i]):int(o[i + 1])].tobytes().decode() for i in range(o.size - 1)] + ["A" * 400, "ACGT" * 3]
    bases, off = oracle.concat([s.encode() for s in seqs])
    canon = oracle.kmer_hashes(bases, off, ktype, k, A.FHASH_CANON_VALUE)
    keep = np.zeros(canon.size, bool)
    for i in range(off.size - 1):
        keep[int(off[i]):int(off[i]) + max(int(off[i + 1]) - int(off[i]) - k + 1, 0)] = True
    occ = canon[keep].astype(np.uint64)
    oc = oracle.Counter(ktype, k, 16, 1 << 20)
    oc.add_reads(bases, off)
    uk, uc = oc.dump(1)
    ob, oo = synth.genome_reads(10, np.full(10, 100, np.int64), 5_000, 0xB2)
    ocanon = oracle.kmer_hashes(ob, oo, ktype, k, A.FHASH_CANON_VALUE)
    ask = np.concatenate([uk, ocanon[:100 - k + 1].astype(np.uint64)])
    (tmp_path / "reads.txt").write_text("%d %d %d\n" % (k, bits, hashes) + "\n".join(seqs) + "\n")
    (tmp_path / "ask.txt").write_text("\n".join(str(int(v)) for v in ask) + "\n")
    r = subprocess.run([test_bin, str(tmp_path / "reads.txt"), str(tmp_path / "ask.txt")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok test_kfilter" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    got = {"passed": [], "info": [], "word": [], "class": [], "entry": [], "held": []}
    for line in r.stdout.splitlines():
        word, _, rest = line.partition(" ")
        if word in got:
            got[word].append(tuple(int(v) for v in rest.split()))
    n_cells = M.cells_for(occ.size, bits)
    planes = M.build(occ, n_cells, hashes)
    assert got["info"] == [(n_cells, occ.size, M.popcount(planes[0]), M.popcount(planes[1]))]
    assert np.array_equal(np.array([w for (w,) in got["word"]], np.uint64), M.words(planes))
    assert [c for _, c in got["class"]] == M.classes(planes, ask, hashes).tolist() and [v for v, _ in got["class"]] == ask.tolist()
    passing = M.classes(planes, uk, hashes) == 2
    assert passing[uc >= 2].all()
    assert got["passed"] == [(int(uc[passing].sum()),)]
    assert got["entry"] == [(int(v), int(c)) for v, c in zip(uk[uc >= 2], uc[uc >= 2])]  # (16-bit counters: the poly-A count as it is)
    assert got["held"] == [(int(passing.sum()), int((uc[passing] == 1).sum()))]

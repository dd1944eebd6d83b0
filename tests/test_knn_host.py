"""-m "not gpu": the host side of the nearest-neighbour feature -- the neighbour file, the `ann` command line of both
datasketcher front ends (refused before a device is touched), and the binding's view of include/kmu.h."""
import os
import re
import subprocess

import numpy as np
import pytest

from kmerutils_amd import _abi as A
from kmerutils_amd import formats as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_neighbour_file_roundtrip_and_truncation(tmp_path):
    fn = str(tmp_path / "out-ann")
    idx = np.array([[3, 1, A.KNN_NONE], [0, A.KNN_NONE, A.KNN_NONE]], np.uint32)
    eq = np.array([[200, 17, 0], [5, 0, 0]], np.uint16)
    F.write_neighbour_file(fn, idx, eq, 200)
    raw = open(fn, "rb").read()
    assert len(raw) == 20 + 6 * 4 + 6 * 2
    assert raw[:20] == np.array([F.MAGIC_NEIGHBOURS], "<u4").tobytes() + np.array([2], "<u8").tobytes() + \
        np.array([3, 200], "<u4").tobytes()
    gi, ge, m = F.read_neighbour_file(fn)
    assert m == 200 and gi.dtype == np.uint32 and ge.dtype == np.uint16
    assert np.array_equal(gi, idx) and np.array_equal(ge, eq)
    open(fn, "wb").write(raw[:-1])
    with pytest.raises(IOError):
        F.read_neighbour_file(fn)
    open(fn, "wb").write(b"\x00" * 40)
    with pytest.raises(IOError):
        F.read_neighbour_file(fn)
    F.write_neighbour_file(fn, np.zeros((0, 4), np.uint32), np.zeros((0, 4), np.uint16), 64)  # no rows
    gi, ge, m = F.read_neighbour_file(fn)
    assert gi.shape == (0, 4) and ge.shape == (0, 4) and m == 64
    with pytest.raises(ValueError):
        F.write_neighbour_file(fn, idx, eq[:1], 200)


BASE = ["-f", "/nonexistent.fastq", "-k", "8", "-s", "200", "-d", "/nonexistent/out"]


def test_python_datasketcher_parses_ann():
    from kmerutils_amd import datasketcher
    a = datasketcher.parse_args(BASE + ["ann", "--nb", "5"])
    assert a.command == "ann" and a.nb == 5
    assert datasketcher.parse_args(BASE + ["-b", "1000", "ann", "-n", "64"]).nb == 64
    assert datasketcher.parse_args(BASE).command is None
    for bad in ("0", "65", "-3"):
        with pytest.raises(SystemExit) as e:
            datasketcher.main(BASE + ["ann", "--nb", bad])  # argparse's exit, before any Context exists
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        datasketcher.parse_args(BASE + ["ann"])


def test_cpp_datasketcher_parses_ann():
    import torch
    from kmerutils_amd import build as kbuild
    kbuild.build_host()
    exe = os.path.join(ROOT, "kmerutils_amd", "bin", "datasketcher")
    for bad in (["ann", "--nb", "0"], ["ann", "-n", "65"], ["ann"], ["--nb", "5"]):
        r = subprocess.run([exe] + BASE + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "usage" in r.stderr and "no CPU fallback" not in r.stderr, (bad, r.stderr)
    if not torch.cuda.is_available():  # a good command line gets as far as the device
        for good in (["ann", "--nb", "5"], ["ann", "-n", "64"]):
            r = subprocess.run([exe] + BASE + good, capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and "no CPU fallback" in r.stderr, (good, r.stderr)


def test_binding_carries_the_header_constants():
    from kmerutils_amd import lib
    txt = open(os.path.join(ROOT, "include", "kmu.h")).read()
    max_k = int(re.search(r"#define\s+KMU_KNN_MAX_K\s+(\d+)", txt).group(1))
    none = int(re.search(r"#define\s+KMU_KNN_NONE\s+(0x[0-9A-Fa-f]+)u", txt).group(1), 16)
    assert (A.KNN_MAX_K, A.KNN_NONE) == (max_k, none) == (64, 0xFFFFFFFF)
    assert F.KNN_NONE == none
    assert "kmu_sig_knn" in lib.SYMBOLS
    assert re.search(r"\bint\s+kmu_sig_knn\s*\(", txt)

"""-m "not gpu": the recurrence of k_chain_align without a device.  tests/cpp/sim_chain_align.cpp drives the functions of
kmerutils_amd/csrc/kmu_align_core.h -- the code the kernel is made of -- over 64 simulated lanes and compares every chain with a
full-matrix banded DP; g++ only, no libkmu."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_chain_align.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "sim_chain_align")


def test_simulated_wave_equals_the_full_matrix():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", SRC, "-o", BIN])
    r = subprocess.run([BIN, "400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_chain_align"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 800  # chains times instances

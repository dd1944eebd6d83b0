"""-m "not gpu": the direction bits, their layout and the walk of kmu_chain_cigar without a device.  tests/cpp/sim_chain_cigar.cpp
drives the functions of kmerutils_amd/csrc/kmu_align_core.h -- the code k_cigar_sweep and k_cigar_walk are made of -- over 64
simulated lanes, writes the trace words into a host buffer, walks them block by block and compares the runs of every chain with a
backtrack over a full matrix by the value rule of include/kmu.h; g++ only, no libkmu."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_chain_cigar.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "sim_chain_cigar")


def test_simulated_trace_and_walk_equal_the_full_matrix_backtrack():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", SRC, "-o", BIN])
    r = subprocess.run([BIN, "400"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_chain_cigar"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 1500  # chains times instances

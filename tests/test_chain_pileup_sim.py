"""-m "not gpu": the tiles, the columns and the per-run votes of kmu_chain_pileup without a device.  tests/cpp/sim_chain_pileup.cpp
drives the functions of kmerutils_amd/csrc/kmu_pile_core.h -- the code k_pile_starts, k_pile_vote and k_pile_call are made of -- over
64 simulated lanes on random run lists, checks that every base and every run is voted exactly once and inside its segment, and
compares the tables with a straight replay of the runs; g++ only, no libkmu."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sim_chain_pileup.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "sim_chain_pileup")


def test_simulated_tiles_and_columns_equal_the_replay():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", SRC, "-o", BIN])
    r = subprocess.run([BIN, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_chain_pileup"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 50000  # runs of all chains, and rows of the call rule

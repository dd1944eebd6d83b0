"""Build tests/cpp/test_unitig_map (test infrastructure, like build_clean.py; the program links libkmu.so only) and
tests/cpp/sim_unitig_map (g++ only: kmu_um_core.h over simulated lanes, no libkmu)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TEST_BIN = os.path.join(HERE, "_build", "test_unitig_map")
SIM_SRC = os.path.join(HERE, "sim_unitig_map.cpp")
SIM_BIN = os.path.join(HERE, "_build", "sim_unitig_map")
SIM_DEPS = [SIM_SRC, os.path.join(ROOT, "include", "kmu.h"), os.path.join(ROOT, "kmerutils_amd", "csrc", "kmu_um_core.h")]


def build_sim(force=False, extra=(), out=SIM_BIN):
    """extra: further compiler flags, such as a sanitizer's, for a binary of another name"""
    if not force and os.path.exists(out) and all(os.path.getmtime(d) <= os.path.getmtime(out) for d in SIM_DEPS):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *extra, SIM_SRC, "-o", out])
    return out


def build(force=False, verbose=False):
    from kmerutils_amd import build as kbuild
    kbuild.build()
    build_sim(force=force)
    return kbuild.compile_host(os.path.join(HERE, "test_unitig_map.cpp"), TEST_BIN, force=force, verbose=verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

"""Build tests/cpp/test_syncmers (test infrastructure, like build_minimizers.py; this program carries its own reference and
links libkmu.so only)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
TEST_BIN = os.path.join(HERE, "_build", "test_syncmers")


def build(force=False, verbose=False):
    from kmerutils_amd import build as kbuild
    kbuild.build()
    return kbuild.compile_host(os.path.join(HERE, "test_syncmers.cpp"), TEST_BIN, force=force, verbose=verbose)


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))

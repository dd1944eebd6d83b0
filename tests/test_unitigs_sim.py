"""-m "not gpu": the kernels of the unitig layout without a device.  tests/cpp/sim_unitigs.cpp drives the functions of
kmerutils_amd/csrc/kmu_ut_core.h and kmu_gather_core.h -- the code the kernels of kmu_unitigs.hip are made of -- over simulated lanes: the links, the mate
test, the doubling rounds from one buffer into the other, the cut of the cycles, the tails, the scans and the write against a
sequential walk on random forests of paths and cycles (paths of 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129 and 1025 reads among them),
every planted arc fault against its refusal, and the tile walk of the sequence copy against a byte loop; g++ only, no libkmu.  The
same program built with AddressSanitizer + UndefinedBehaviorSanitizer runs as a stand-alone child process on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_unitigs  # noqa: E402  (tests/cpp/build_unitigs.py)


def test_simulated_unitigs_equal_the_walk():
    import subprocess
    sim = build_unitigs.build_sim()
    r = subprocess.run([sim, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_unitigs"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 300000  # unitigs, steps, places, refusals and copied bytes of all cases


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_simulation_runs_clean_under_the_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them, as tests/test_host_san.py does)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    sim = build_unitigs.build_sim(force=True, extra=SAN if linked else (), out=str(tmp_path / "sim_unitigs_san"))
    r = subprocess.run([sim, "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_unitigs") and "runtime error" not in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]

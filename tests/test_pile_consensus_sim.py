"""-m "not gpu": the slots, the votes and the row rule of read correction without a device.  tests/cpp/sim_pile_consensus.cpp drives
the functions of kmerutils_amd/csrc/kmu_cons_core.h -- the code k_ins_plan, k_ins_vote and the consensus kernels are made of -- over
64 simulated lanes on random run lists and random tables: every inserted letter within a row's slots is voted exactly once and
inside the row's slots, the block-offset lookup equals the full prefix sum, the row lengths sum to the total and the written bytes
equal a straight replay; g++ only, no libkmu.  The same program built with AddressSanitizer + UndefinedBehaviorSanitizer runs as a
stand-alone child process on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_pile_consensus  # noqa: E402  (tests/cpp/build_pile_consensus.py)


def test_simulated_votes_and_rows_equal_the_replay():
    import subprocess
    sim = build_pile_consensus.build_sim()
    r = subprocess.run([sim, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_pile_consensus"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 100000  # runs, voted letters, rows and output bytes of all cases


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_simulation_runs_clean_under_the_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them, as tests/test_host_san.py does)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    sim = build_pile_consensus.build_sim(force=True, extra=SAN if linked else (), out=str(tmp_path / "sim_pile_consensus_san"))
    r = subprocess.run([sim, "200"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_pile_consensus") and "runtime error" not in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]

"""-m "not gpu": the kernels of the string graph without a device.  tests/cpp/sim_string_graph.cpp drives the functions of
kmerutils_amd/csrc/kmu_sg_core.h -- the code k_sg_classify, k_sg_arcs, k_sg_heads and k_sg_reduce are made of -- over 64 simulated
lanes: the classifier and the range checks against a replay of the contract, the arc pair and the compaction, the slice and run
searches against linear scans (runs of duplicate arcs, runs that start at index 0 or end at the last arc), and the marks of the
simulated waves against a brute-force triple loop; g++ only, no libkmu.  The same program built with AddressSanitizer +
UndefinedBehaviorSanitizer runs as a stand-alone child process on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_string_graph  # noqa: E402  (tests/cpp/build_string_graph.py)


def test_simulated_graph_equals_the_brute_force():
    import subprocess
    sim = build_string_graph.build_sim()
    r = subprocess.run([sim, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_string_graph"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 300000  # records, arcs, searches and marks of all cases


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_simulation_runs_clean_under_the_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them, as tests/test_host_san.py does)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    sim = build_string_graph.build_sim(force=True, extra=SAN if linked else (), out=str(tmp_path / "sim_string_graph_san"))
    r = subprocess.run([sim, "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_string_graph") and "runtime error" not in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]

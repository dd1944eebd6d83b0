"""-m "not gpu": the kernels of the unitig map without a device.  tests/cpp/sim_unitig_map.cpp drives the functions of
kmerutils_amd/csrc/kmu_um_core.h -- the code the kernels of kmu_unitig_map.hip are made of -- over simulated lanes in launch order,
once ascending and once descending: the checks, the candidates with their atomic maximum, the flags, the scan and the records against
a sequential restatement of the contract on random forests of paths and cycles with planted containments, and every planted fault
against its refusal; g++ only, no libkmu.  The same program built with AddressSanitizer + UndefinedBehaviorSanitizer runs as a
stand-alone child process on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_unitig_map  # noqa: E402  (tests/cpp/build_unitig_map.py)


def test_simulated_map_equals_the_contract():
    import subprocess
    sim = build_unitig_map.build_sim()
    r = subprocess.run([sim, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_unitig_map"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 100000  # records, stats and refusals of all cases


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_simulation_runs_clean_under_the_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them, as tests/test_host_san.py does)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    sim = build_unitig_map.build_sim(force=True, extra=SAN if linked else (), out=str(tmp_path / "sim_unitig_map_san"))
    r = subprocess.run([sim, "60"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_unitig_map") and "runtime error" not in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]

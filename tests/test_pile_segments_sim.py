"""-m "not gpu": the segment pass and the range copy of read trimming without a device.  tests/cpp/sim_pile_segments.cpp drives the
functions of kmerutils_amd/csrc/kmu_seg_core.h and kmu_gather_core.h -- the code k_seg_count, k_seg_write, k_seg_keep, k_seg_reads and
k_ext_copy are made of -- over 64 simulated lanes on random tables: starts and ends pair up, the runs equal a straight per-read replay, every row is in
at most one run and no run crosses a read boundary, the summaries equal the replay's, and every output byte of the copy is written
exactly once from the range that holds it; g++ only, no libkmu.  The same program built with AddressSanitizer +
UndefinedBehaviorSanitizer runs as a stand-alone child process on the CPU."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "cpp"))
import build_trim  # noqa: E402  (tests/cpp/build_trim.py)


def test_simulated_segments_equal_the_replay():
    import subprocess
    sim = build_trim.build_sim()
    r = subprocess.run([sim, "300"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_pile_segments"), r.stdout[-1000:] + r.stderr[-1000:]
    assert int(r.stdout.split()[-1]) > 100000  # rows, runs, output bytes and ranges of all cases


SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_simulation_runs_clean_under_the_sanitizers(tmp_path):
    import subprocess
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them, as tests/test_host_san.py does)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    sim = build_trim.build_sim(force=True, extra=SAN if linked else (), out=str(tmp_path / "sim_pile_segments_san"))
    r = subprocess.run([sim, "100"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok sim_pile_segments") and "runtime error" not in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]

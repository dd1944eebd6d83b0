"""The host-only C++ of the project under AddressSanitizer + UndefinedBehaviorSanitizer: tests/cpp/test_host_san.cpp (packed
sequences, k-mer values, the file readers and writers of include/kmerutils.hpp, the chunk plan of the host pipeline and the
plans of the partitioned count build) compiled as a stand-alone program with g++ and run as a child process.  No GPU, no libkmu."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_host_code_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    exe = tmp_path / "test_host_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + (SAN if linked else []) + ["-Wall", "-Wextra", "-pthread", os.path.join(HERE, "cpp", "test_host_san.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr

"""The sub-list rule of k_multiset_long (PMH_LONG_TP, pmh_long_parts, pmh_long_part_of in kmu_sketch_host.hpp) on the host: the
stand-alone program tests/cpp/test_long_parts.cpp, compiled for the host alone (no device needed) and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_parts_program(tmp_path):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "test_long_parts")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "cpp", "test_long_parts.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "test_long_parts ok" in out.stdout, out.stdout + out.stderr

"""The launch plan of k_sketch_super (SuperPlan, super_plan in kmu_sketch_host.hpp) on the host: the stand-alone program
tests/cpp/test_super_plan.cpp, compiled for the host alone (no device needed) and run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_super_plan_program(tmp_path):
    hipcc = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "test_super_plan")
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function",
                           os.path.join(ROOT, "tests", "cpp", "test_super_plan.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "test_super_plan ok" in out.stdout, out.stdout + out.stderr

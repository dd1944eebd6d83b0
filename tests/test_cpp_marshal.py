"""What every wrapper of include/kmerutils.hpp hands to the C-ABI: tests/cpp/test_marshal.cpp defines recording stand-ins for the
kmu_* entry points, runs the wrappers on small inputs and prints one line per library call.  tests/cpp/marshal_calls.txt is that
output, recorded once from the header before its marshalling steps were written once; it is not regenerated from a later header.
The program is stand-alone (g++, no GPU, no libkmu) and runs as a child process, once plain and once under AddressSanitizer +
UndefinedBehaviorSanitizer with libstdc++'s assertions."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "cpp", "test_marshal.cpp")
RECORDED = os.path.join(HERE, "cpp", "marshal_calls.txt")
PLAIN = ["-std=c++17", "-Wall", "-Wextra"]
SAN = ["-O1", "-g", "-D_GLIBCXX_ASSERTIONS", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def trace(tmp_path, name, flags):
    exe = tmp_path / name
    r = subprocess.run(["g++"] + PLAIN + flags + ["-I", os.path.join(ROOT, "include"), SOURCE, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    print(name + ":", r.stderr.strip())
    return r.stdout.splitlines()


def same_as_recorded(got):
    with open(RECORDED) as f:
        want = f.read().splitlines()
    case = ""
    for i, (g, w) in enumerate(zip(got, want)):
        if w.startswith("# "):
            case = w
        assert g == w, "line %d, in %s:\n  recorded: %s\n  now:      %s" % (i + 1, case, w, g)
    assert len(got) == len(want), "%d lines, %d recorded; the first one over: %s" % (len(got), len(want), (got + want)[min(len(got), len(want))])


def test_wrappers_pass_what_was_recorded(tmp_path):
    same_as_recorded(trace(tmp_path, "test_marshal", []))


def test_wrappers_pass_what_was_recorded_under_the_sanitizers(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # (a machine whose g++ has no sanitizer runtimes to link: the same program without them)
    linked = subprocess.run(["g++", "-std=c++17"] + SAN + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0
    print("sanitizer runtimes:", "linked" if linked else "absent, plain build")
    same_as_recorded(trace(tmp_path, "test_marshal_san", SAN if linked else []))

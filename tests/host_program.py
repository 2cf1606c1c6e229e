"""The stand-alone host programs of erased-cells_amd/host (headers of csrc/ alone: no library, no GPU, nothing loaded into Python):
one way to build and run them for the tests that do."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "erased-cells_amd", "host")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def run_host_program(target, *args, timeout=300, stdin=None, passed="checks passed", check=True):
    """Builds `target` of host/Makefile afresh with the ROCm clang (the plain, the _san and the _tsan forms alike), runs it with
    `args` and `stdin` under `timeout` seconds, and asserts that it exited with 0, that no sanitizer reported anything and that it
    printed `passed` (check=False: only that it built).  Returns the finished process for the caller's own assertions."""
    b = subprocess.run(["make", "-C", HOST, "-s", "-B", "CXX=" + CLANG, "SAN_CXX=" + CLANG, "TSAN_CXX=" + CLANG, target], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(HOST, target), *args], input=stdin, capture_output=True, text=True, timeout=timeout)
    if not check:
        return r
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert passed in r.stdout, r.stdout[-2000:]
    return r

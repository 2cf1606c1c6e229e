"""The reductions' launch plan (erased-cells_amd/csrc/ec_reduce_plan.hpp) run on its own by
erased-cells_amd/host/test_reduce_plan.cpp: reduce_plan() against the arithmetic of the three launchers it replaced, kept in the
test as the frozen specification, over pointer offsets, cell sizes, lengths around every threshold, the launch shapes and the
knobs — built with the ROCm clang, plain and under the address and undefined-behaviour sanitizers.  A stand-alone program:
nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "erased-cells_amd", "host")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def _build_and_run(target):
    b = subprocess.run(["make", "-C", HOST, "-s", "-B", "CXX=" + CLANG, "SAN_CXX=" + CLANG, target], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)


def test_reduce_plan_matches_the_three_launchers_it_replaced():
    r = _build_and_run("test_reduce_plan")
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_reduce_plan_under_the_address_and_undefined_behaviour_sanitizers():
    r = _build_and_run("test_reduce_plan_san")
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr

"""The cut of a job of more tiles than one launch holds into launches (erased-cells_amd/csrc/ec_launch_split.hpp) run on its own by
erased-cells_amd/host/test_launch_split.cpp: for tile counts around 2^24, 2^25 and 2^31 - 1 the launches cover every tile exactly
once and none holds more workgroups than a dispatch can — built with the ROCm clang, plain and under the address and
undefined-behaviour sanitizers.  A stand-alone program: nothing of it is loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "erased-cells_amd", "host")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def _build_and_run(target):
    b = subprocess.run(["make", "-C", HOST, "-s", "-B", "CXX=" + CLANG, "SAN_CXX=" + CLANG, target], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)


def test_the_launches_cover_every_tile_once_within_the_cap():
    r = _build_and_run("test_launch_split")
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers():
    r = _build_and_run("test_launch_split_san")
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr

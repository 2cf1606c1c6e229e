"""erased-cells_amd/host/test_stack_plan.cpp: the refusals ec_composite and ec_composite_rank share (csrc/ec_stack_plan.hpp) in either
entry point's order and with their exact texts, for stacks of 1, 3 and 64 layers, at 2^31 - 1 and 2^31 tiles, for an empty stack with
null pointers and for 2^62 cells; the argument block's head and its alignment test.  A stand-alone program, built plainly and with
-fsanitize=address,undefined.  Needs no device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("target", ["test_stack_plan", "test_stack_plan_san"])
def test_the_plan_header_alone_and_under_sanitizers(target):
    host = os.path.join(ROOT, "erased-cells_amd", "host")
    clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    b = subprocess.run(["make", "-C", host, "-s", "-B", "CXX=" + clang, "SAN_CXX=" + clang, target], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([os.path.join(host, target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    assert "checks passed" in r.stdout

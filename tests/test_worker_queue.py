"""The shard group's launch-thread queue (erased-cells_amd/csrc/ec_worker.hpp) run on its own by
erased-cells_amd/host/test_worker_queue.cpp: four workers fed 50,000 jobs each by one posting thread that catches them
polling and asleep, a stop with jobs still queued, and the latch — built with the ROCm clang, plain and under the thread
sanitizer.  A stand-alone program: nothing of it is loaded into Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "erased-cells_amd", "host")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")


def _build_and_run(target):
    b = subprocess.run(["make", "-C", HOST, "-s", "-B", "CXX=" + CLANG, "TSAN_CXX=" + CLANG, target], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    return subprocess.run([os.path.join(HOST, target)], capture_output=True, text=True, timeout=300)


def test_worker_queue_keeps_order_drains_on_stop_and_the_latch_waits():
    r = _build_and_run("test_worker_queue")
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


def test_worker_queue_under_the_thread_sanitizer():
    r = _build_and_run("test_worker_queue_tsan")
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr:  # the runtime could not start on this kernel: nothing ran
        pytest.skip("thread sanitizer runtime: " + r.stderr.strip().splitlines()[0])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr

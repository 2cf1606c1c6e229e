"""The shard group's launch-thread queue (erased-cells_amd/csrc/ec_worker.hpp) run on its own by
erased-cells_amd/host/test_worker_queue.cpp: four workers fed 50,000 jobs each by one posting thread that catches them
polling and asleep, a stop with jobs still queued, and the latch — built with the ROCm clang, plain and under the thread
sanitizer.  A stand-alone program: nothing of it is loaded into Python."""
import pytest

from host_program import run_host_program


def test_worker_queue_keeps_order_drains_on_stop_and_the_latch_waits():
    run_host_program("test_worker_queue", passed="all checks passed")


def test_worker_queue_under_the_thread_sanitizer():
    r = run_host_program("test_worker_queue_tsan", check=False)
    if r.returncode != 0 and "unexpected memory mapping" in r.stderr:  # the runtime could not start on this kernel: nothing ran
        pytest.skip("thread sanitizer runtime: " + r.stderr.strip().splitlines()[0])
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert "ThreadSanitizer" not in r.stderr, r.stderr

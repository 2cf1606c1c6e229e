"""The reductions' launch plan (erased-cells_amd/csrc/ec_reduce_plan.hpp) run on its own by
erased-cells_amd/host/test_reduce_plan.cpp: reduce_plan() against the arithmetic of the three launchers it replaced, kept in the
test as the frozen specification, over pointer offsets, cell sizes, lengths around every threshold, the launch shapes and the
knobs — built with the ROCm clang, plain and under the address and undefined-behaviour sanitizers.  A stand-alone program:
nothing of it is loaded into Python."""
from host_program import run_host_program


def test_reduce_plan_matches_the_three_launchers_it_replaced():
    run_host_program("test_reduce_plan", passed="all checks passed")


def test_reduce_plan_under_the_address_and_undefined_behaviour_sanitizers():
    run_host_program("test_reduce_plan_san", passed="all checks passed")

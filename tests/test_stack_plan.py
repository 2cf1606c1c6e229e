"""erased-cells_amd/host/test_stack_plan.cpp: the refusals ec_composite and ec_composite_rank share (csrc/ec_stack_plan.hpp) in either
entry point's order and with their exact texts, for stacks of 1, 3 and 64 layers, at 2^31 - 1 and 2^31 tiles, for an empty stack with
null pointers and for 2^62 cells; the argument block's head and its alignment test.  A stand-alone program, built plainly and with
-fsanitize=address,undefined.  Needs no device."""
import pytest

from host_program import run_host_program


@pytest.mark.parametrize("target", ["test_stack_plan", "test_stack_plan_san"])
def test_the_plan_header_alone_and_under_sanitizers(target):
    run_host_program(target)

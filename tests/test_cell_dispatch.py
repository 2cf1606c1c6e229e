"""The cell-type dispatcher every type-erased entry point goes through (csrc/ec_dispatch.hpp over the type list of
csrc/ec_lattice.hpp), alone and without a GPU.

erased-cells_amd/host/test_cell_dispatch.cpp includes the two headers and nothing else of the library: each code 0..9 reaches
its C type exactly once, all 100 pairs in argument order, the codes -1, 10, 255 and INT_MAX reach nothing (alone and in either
position of a pair) and give the fallback back, the widths 1, 2, 4, 8 give the unsigned word of that size, and the type <-> code
maps are each other's inverse (static_assert).  Built plain and under the address and undefined-behaviour sanitizers.  A
stand-alone program: nothing of it is loaded into Python.
"""
import pytest

from host_program import run_host_program


@pytest.mark.parametrize("target", ["test_cell_dispatch", "test_cell_dispatch_san"])
def test_dispatcher_from_the_headers_alone(target):
    r = run_host_program(target, passed="cell dispatch ok")
    assert r.stdout.strip().split("\n")[-1] == "cell dispatch ok", r.stdout[-2000:]

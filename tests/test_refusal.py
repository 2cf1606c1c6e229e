"""What the raster families' argument checks share (erased-cells_amd/csrc/ec_refusal.hpp) run on its own by
erased-cells_amd/host/test_refusal.cpp: the interval test on blocks that touch, nest, are equal, are absent or empty or end at the
last address, the walk over a table of overlaps, the alignment test on an absent pointer — plain and under the address and
undefined-behaviour sanitizers.  A stand-alone program: nothing of it is loaded into Python.  The families' own refusals run in
the same way in test_regions_args.py, test_distance_args.py, test_zonal_args.py and test_reclass_args.py."""
import pytest

from host_program import run_host_program


@pytest.mark.parametrize("target", ["test_refusal", "test_refusal_san"])
def test_the_refusal_header_alone_and_under_sanitizers(target):
    run_host_program(target)

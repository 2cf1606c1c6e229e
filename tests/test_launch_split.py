"""The cut of a job of more tiles than one launch holds into launches (erased-cells_amd/csrc/ec_launch_split.hpp) run on its own by
erased-cells_amd/host/test_launch_split.cpp: for tile counts around 2^24, 2^25 and 2^31 - 1 the launches cover every tile exactly
once and none holds more workgroups than a dispatch can — built with the ROCm clang, plain and under the address and
undefined-behaviour sanitizers.  A stand-alone program: nothing of it is loaded into Python."""
from host_program import run_host_program


def test_the_launches_cover_every_tile_once_within_the_cap():
    run_host_program("test_launch_split", passed="all checks passed")


def test_the_same_under_the_address_and_undefined_behaviour_sanitizers():
    run_host_program("test_launch_split_san", passed="all checks passed")

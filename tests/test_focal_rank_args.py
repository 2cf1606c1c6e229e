"""Every refusal of ec_focal_rank / ec_focal_majority (include/erased_cells.h) in the stated order, each decided before the library
asks for a device: this file needs none.  Only calls that are refused, or that have nothing to do, are made — the pointers are
addresses that are never dereferenced.  Also here: the spellings the Python mirror accepts, that the tile size the tests restate
(tests/focal_rank_cases.py) is the one the kernels are built with, and the per-cell header alone as a stand-alone program, built plainly
and with the address and undefined-behaviour sanitizers."""
import os
import re

import pytest

import focal_rank_cases as K
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
SRC, DST, SMASK, DMASK = 0x10000, 0x20000, 0x30000, 0x40000   # never dereferenced
WHOLE = 1


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def rank(L, t=1, src=SRC, smask=None, cols=100, rows=50, rx=1, ry=1, num=1, den=2, method=0, flags=0, dst=DST, dmask=None):
    return L.ec_focal_rank(t, src, smask, cols, rows, rx, ry, num, den, method, flags, dst, dmask, None)


def majority(L, t=1, src=SRC, smask=None, cols=100, rows=50, rx=1, ry=1, flags=0, dst=DST, dmask=None):
    return L.ec_focal_majority(t, src, smask, cols, rows, rx, ry, flags, dst, dmask, None)


# in the order of the header; every later entry is still wrong in every call of the order test below
REFUSALS = [
    ("null src", dict(src=None), "null pointer"),
    ("null dst", dict(dst=None), "null pointer"),
    ("unknown flag bit 4", dict(flags=4), "unknown flag bits"),
    ("EC_FOCAL_NORMALIZE is no flag here", dict(flags=2), "unknown flag bits"),
    ("unknown flag bit 2^31", dict(flags=1 << 31), "unknown flag bits"),
    ("rx above the cap", dict(rx=8), "EC_FOCAL_RADIUS_CAP"),
    ("ry above the cap", dict(ry=8), "EC_FOCAL_RADIUS_CAP"),
    ("rx far above the cap", dict(rx=0xffffffff), "EC_FOCAL_RADIUS_CAP"),
    ("9 x 9", dict(rx=4, ry=4), "EC_FOCAL_RANK_MAX_TAPS"),
    ("15 x 5", dict(rx=7, ry=2), "EC_FOCAL_RANK_MAX_TAPS"),
    ("5 x 15", dict(rx=2, ry=7), "EC_FOCAL_RANK_MAX_TAPS"),
    ("15 x 15", dict(rx=7, ry=7), "EC_FOCAL_RANK_MAX_TAPS"),
    ("a source mask and no dst_mask", dict(smask=SMASK), "dst_mask is NULL"),
    ("WHOLE and no dst_mask", dict(flags=WHOLE), "dst_mask is NULL"),
    ("cols * rows beyond 64 bits", dict(cols=1 << 33, rows=1 << 31), "overflows 64 bits"),
    ("dst == src", dict(dst=SRC), "dst == src"),
    ("dst_mask == src_mask", dict(smask=SMASK, dmask=SMASK), "dst_mask == src_mask"),
    ("2^31 tiles in one row of tiles", dict(cols=K.TW << 31, rows=1), "2^31 - 1 tiles"),
    ("2^32 tiles", dict(cols=K.TW << 20, rows=K.TH << 12), "2^31 - 1 tiles"),
    ("2^31 tiles in one column of tiles", dict(cols=1, rows=K.TH << 31), "2^31 - 1 tiles"),
]
RANK_ONLY = [
    ("den 0", dict(den=0), "EC_RANK_MAX_DEN"),
    ("den above the cap", dict(den=65536), "EC_RANK_MAX_DEN"),
    ("num > den", dict(num=3, den=2), "num <= den"),
    ("method 2", dict(method=2), "ec_rank_method"),
    ("method -1", dict(method=-1), "ec_rank_method"),
]
ENTRIES = (("ec_focal_rank", rank), ("ec_focal_majority", majority))


def refused(L, name, call, what, kw, text):
    assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
    assert call(L, **kw) == ARG, (name, what)
    msg = L.ec_last_error_string().decode()
    assert msg.startswith(name + ": ") and text in msg, (name, what, msg)


def test_every_refusal_of_both_entry_points(ec):
    L = ec.lib()
    for what, kw, text in REFUSALS:
        for name, call in ENTRIES:
            refused(L, name, call, what, kw, text)
    for what, kw, text in RANK_ONLY:
        refused(L, "ec_focal_rank", rank, what, kw, text)
    for radius in K.REFUSED_RADII:
        for name, call in ENTRIES:
            refused(L, name, call, radius, dict(rx=radius[0], ry=radius[1]), "EC_FOCAL_RANK_MAX_TAPS")


# one representative of each step of the order, first to last
ORDER = [("null pointer", dict(src=None)), ("unknown flag bits", dict(flags=8)), ("EC_FOCAL_RADIUS_CAP", dict(rx=9)),
         ("EC_FOCAL_RANK_MAX_TAPS", dict(rx=4, ry=5)), ("dst_mask is NULL", dict(smask=SMASK, dmask=None)),
         ("overflows 64 bits", dict(cols=1 << 33, rows=1 << 31)), ("dst == src", dict(dst=SRC)), ("2^31 - 1 tiles", dict(cols=K.TW << 31, rows=1)),
         ("EC_RANK_MAX_DEN", dict(den=0)), ("ec_rank_method", dict(method=7))]


def test_the_order_of_the_refusals(ec):
    """with the mistakes of steps i, i + 1, .. all made at once, the text is step i's.  (A call cannot make every mistake at once — a
    radius has one value — so where two steps want the same argument the later one gives way.)"""
    L = ec.lib()
    for name, call in ENTRIES:
        steps = ORDER if call is rank else ORDER[:8]
        for i, (text, _) in enumerate(steps):
            kw = {}
            for _, later in reversed(steps[i:]):
                kw.update(later)            # the earliest step's arguments win
            assert call(L, **kw) == ARG
            msg = L.ec_last_error_string().decode()
            assert msg.startswith(name + ": ") and text in msg, (name, text, msg, kw)


def test_a_bad_dtype_is_unsupported_type(ec):
    L = ec.lib()
    for bad in (10, 255):
        for name, call in ENTRIES:
            assert call(L, t=bad) == UNSUPPORTED
            assert L.ec_last_error_string().decode() == f"{name}: bad dtype {bad}"
            assert call(L, t=bad, cols=0) == UNSUPPORTED   # also for an empty raster
            assert call(L, t=bad, rx=8) == ARG             # the refusals come first


def test_an_empty_raster_is_ok_and_launches_nothing(ec):
    L = ec.lib()
    for cols, rows in ((0, 0), (0, 7), (7, 0)):
        for t in range(10):
            for radius in K.RADII:
                assert rank(L, t=t, cols=cols, rows=rows, rx=radius[0], ry=radius[1]) == OK
                assert majority(L, t=t, cols=cols, rows=rows, rx=radius[0], ry=radius[1]) == OK
    assert rank(L, cols=0, rows=5, rx=8) == ARG and majority(L, cols=0, rows=5, rx=4, ry=4) == ARG   # the checks come first
    assert rank(L, cols=0, rows=5, den=0) == ARG and rank(L, cols=5, rows=0, method=2) == ARG


def test_every_accepted_footprint_passes_the_checks(ec):
    """every (rx, ry) within the cap: accepted exactly when it has at most 64 cells (an empty raster: nothing is launched)"""
    L = ec.lib()
    for rx in range(8):
        for ry in range(8):
            want = OK if (2 * rx + 1) * (2 * ry + 1) <= K.MAX_TAPS else ARG
            assert rank(L, cols=0, rx=rx, ry=ry) == want and majority(L, cols=0, rx=rx, ry=ry) == want, (rx, ry)
    for fits in ((1, 1), (2, 2), (3, 3), (3, 4), (1, 7), (0, 7)):    # 3 x 3, 5 x 5, 7 x 7, 7 x 9, 3 x 15, 1 x 15
        assert rank(L, cols=0, rx=fits[0], ry=fits[1]) == OK


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    assert ec._ffi.EC_FOCAL_RANK_MAX_TAPS == 64 == K.MAX_TAPS
    for cls in (ec.CellBuffer, ec.MaskedCellBuffer):
        for method in ("focal_rank", "focal_median", "focal_majority"):
            assert callable(getattr(cls, method))
    # q, method and radius are read by the functions composite_rank and focal read theirs with
    assert B._rank_args((1, 2), "lower") == (1, 2, 0) and B._rank_args([9, 10], "upper") == (9, 10, 1)
    assert B._rank_args(0, ec._ffi.EC_RANK_LOWER) == (0, 1, 0) and B._rank_args(1, ec._ffi.EC_RANK_UPPER) == (1, 1, 1)
    assert B._radius((7, 0)) == (7, 0) and B._radius([1, 7]) == (1, 7)
    import inspect
    sig = inspect.signature(ec.CellBuffer.focal_rank).parameters
    assert (sig["q"].default, sig["method"].default, sig["radius"].default, sig["whole"].default) == ((1, 2), "lower", (1, 1), False)
    sig = inspect.signature(ec.MaskedCellBuffer.focal_median).parameters
    assert list(sig)[1:] == ["cols", "radius", "method", "whole"] and (sig["radius"].default, sig["method"].default) == ((1, 1), "lower")
    sig = inspect.signature(ec.CellBuffer.focal_majority).parameters
    assert list(sig)[1:] == ["cols", "radius", "whole"] and sig["radius"].default == (1, 1)


def test_the_tile_size_and_the_caps_the_tests_restate_are_the_kernels(ec):
    csrc = os.path.join(ROOT, "erased-cells_amd", "csrc")
    text = open(os.path.join(csrc, "ec_focal_kernels.hpp")).read()
    tw = re.search(r"constexpr\s+int\s+TW\s*=\s*(\d+)\s*;", text)
    th = re.search(r"constexpr\s+int\s+TH\s*=\s*(\d+)\s*;", text)
    assert tw and th and (int(tw.group(1)), int(th.group(1))) == (K.TW, K.TH)
    assert '#include "ec_focal_kernels.hpp"' in open(os.path.join(csrc, "ec_focal_rank_kernels.hpp")).read()   # the same TW and TH
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_FOCAL_RANK_MAX_TAPS\s*=\s*64\b", header)
    assert re.search(r"kRankMaxTaps\s*=\s*64\b", open(os.path.join(csrc, "ec_focal_plan.hpp")).read())
    assert re.search(r"kFocalRankMaxTaps\s*=\s*64\b", open(os.path.join(csrc, "ec_focal_rank_cell.hpp")).read())
    # the stage and the results of the largest launches (8-byte cells, masked) fit well inside 64 KiB
    pad = lambda b: (b + 15) // 16 * 16
    for rx in range(8):
        for ry in range(8):
            if (2 * rx + 1) * (2 * ry + 1) <= K.MAX_TAPS:
                hr, wide = K.TH + 2 * ry, K.TW + 2 * rx
                assert hr * pad(wide * 8) + hr * pad(wide) + K.TH * K.TW * 8 + pad(K.TH * K.TW) <= 32 * 1024, (rx, ry)


@pytest.mark.parametrize("target", ["test_focal_rank_cell", "test_focal_rank_cell_san"])
def test_the_cell_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_focal_rank_cell.cpp: majority_pick and the rank pick with tap positions from
    csrc/ec_focal_rank_cell.hpp alone, against std::sort and std::map — a stand-alone program, built plainly and with
    -fsanitize=address,undefined"""
    run_host_program(target)

"""Every refusal of ec_focal / ec_focal_convolve (include/erased_cells.h), each decided before the library asks for a device: this file
needs none.  Only calls that are refused, or that have nothing to do, are made — the pointers are addresses that are never
dereferenced.  Also here: ec_focal_result_type, the spellings the Python mirror accepts, and that the tile size the tests restate
(tests/focal_cases.py) is the one the kernels are built with."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import focal_cases as K
from host_program import run_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, UNSUPPORTED, ARG = 0, 2, 6
SRC, DST, SMASK, DMASK = 0x10000, 0x20000, 0x30000, 0x40000   # never dereferenced
WHOLE, NORMALIZE = 1, 2


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def focal(L, op=0, t=1, src=SRC, smask=None, cols=100, rows=50, rx=1, ry=1, flags=0, dst=DST, dmask=None):
    return L.ec_focal(op, t, src, smask, cols, rows, rx, ry, flags, dst, dmask, None)


W9 = (C.c_double * 225)(*([1.0] * 225))


def convolve(L, t=1, src=SRC, smask=None, cols=100, rows=50, w=W9, rx=1, ry=1, flags=0, dst=DST, dmask=None):
    return L.ec_focal_convolve(t, src, smask, cols, rows, w, rx, ry, flags, dst, dmask, None)


REFUSALS = [
    ("null src", dict(src=None), "null pointer"),
    ("null dst", dict(dst=None), "null pointer"),
    ("unknown flag bit 4", dict(flags=4), "unknown flag bits"),
    ("unknown flag bit 2^31", dict(flags=1 << 31), "unknown flag bits"),
    ("rx above the cap", dict(rx=8), "EC_FOCAL_RADIUS_CAP"),
    ("ry above the cap", dict(ry=8), "EC_FOCAL_RADIUS_CAP"),
    ("rx far above the cap", dict(rx=0xffffffff), "EC_FOCAL_RADIUS_CAP"),
    ("a source mask and no dst_mask", dict(smask=SMASK), "dst_mask is NULL"),
    ("WHOLE and no dst_mask", dict(flags=WHOLE), "dst_mask is NULL"),
    ("cols * rows beyond 64 bits", dict(cols=1 << 33, rows=1 << 31), "overflows 64 bits"),
    ("2^31 tiles in one row of tiles", dict(cols=K.TW << 31, rows=1), "2^31 - 1 tiles"),
    ("2^32 tiles", dict(cols=K.TW << 20, rows=K.TH << 12), "2^31 - 1 tiles"),
    ("2^31 tiles in one column of tiles", dict(cols=1, rows=K.TH << 31), "2^31 - 1 tiles"),
    ("dst == src", dict(dst=SRC), "dst == src"),
    ("dst_mask == src_mask", dict(smask=SMASK, dmask=SMASK), "dst_mask == src_mask"),
]


def test_every_refusal_of_both_entry_points(ec):
    L = ec.lib()
    for what, kw, text in REFUSALS:
        for name, call in (("ec_focal", focal), ("ec_focal_convolve", convolve)):
            assert L.ec_tune_set(b"no such knob", 0) == ARG   # another text in between: the next one is this call's own
            assert call(L, **kw) == ARG, (name, what)
            msg = L.ec_last_error_string().decode()
            assert msg.startswith(name + ": ") and text in msg, (name, what, msg)
    for op in (-1, 4, 255):
        assert focal(L, op=op) == ARG and "ec_focal_op" in L.ec_last_error_string().decode(), op
    assert focal(L, flags=NORMALIZE) == ARG and "ec_focal_convolve's" in L.ec_last_error_string().decode()
    assert focal(L, flags=NORMALIZE | WHOLE, dmask=DMASK) == ARG
    assert convolve(L, w=None) == ARG and "null weights" in L.ec_last_error_string().decode()


def test_a_bad_dtype_is_unsupported_type(ec):
    L = ec.lib()
    for bad in (10, 255):
        assert focal(L, t=bad) == UNSUPPORTED
        assert L.ec_last_error_string().decode() == f"ec_focal: bad dtype {bad}"
        assert convolve(L, t=bad) == UNSUPPORTED
        assert L.ec_last_error_string().decode() == f"ec_focal_convolve: bad dtype {bad}"
        assert focal(L, t=bad, cols=0) == UNSUPPORTED   # also for an empty raster


def test_an_empty_raster_is_ok_and_launches_nothing(ec):
    L = ec.lib()
    for cols, rows in ((0, 0), (0, 7), (7, 0)):
        for t in range(10):
            assert focal(L, t=t, cols=cols, rows=rows) == OK
            assert convolve(L, t=t, cols=cols, rows=rows, flags=NORMALIZE) == OK
    assert focal(L, cols=0, rows=5, rx=8) == ARG    # the checks come first


def test_result_type(ec):
    L = ec.lib()
    for t in range(10):
        assert [L.ec_focal_result_type(op, t) for op in range(4)] == [ec.Float64, ec.Float64, t, t]
    assert [L.ec_focal_result_type(op, 0) for op in (-1, 4)] == [255, 255]
    assert [L.ec_focal_result_type(0, t) for t in (10, 255)] == [255, 255]


def test_the_python_spellings(ec):
    from erased_cells_hip import buffer as B
    assert [B._focal_op(s) for s in ("sum", "mean", "min", "max")] == [0, 1, 2, 3] == [B._focal_op(k) for k in range(4)]
    assert (ec._ffi.EC_FOCAL_SUM, ec._ffi.EC_FOCAL_MEAN, ec._ffi.EC_FOCAL_MIN, ec._ffi.EC_FOCAL_MAX) == (0, 1, 2, 3)
    assert (ec._ffi.EC_FOCAL_WHOLE, ec._ffi.EC_FOCAL_NORMALIZE, ec._ffi.EC_FOCAL_RADIUS_CAP) == (1, 2, 7)
    for bad in ("median", "Sum", 4, -1, True, 1.0, None):
        with pytest.raises(ec.EcError):
            B._focal_op(bad)
    for bad in ((-1, 0), (0, -1), (8, 0), (0, 8), (2 ** 32 + 1, 1), (1, 2 ** 32)):   # the last two would wrap to (1, 1) and (1, 0) in a uint32_t
        with pytest.raises(ec.EcError, match="EC_FOCAL_RADIUS_CAP"):
            B._radius(bad)
    assert B._radius((7, 0)) == (7, 0)


def test_the_tile_size_the_tests_restate_is_the_kernels(ec):
    text = open(os.path.join(ROOT, "erased-cells_amd", "csrc", "ec_focal_kernels.hpp")).read()
    tw = re.search(r"constexpr\s+int\s+TW\s*=\s*(\d+)\s*;", text)
    th = re.search(r"constexpr\s+int\s+TH\s*=\s*(\d+)\s*;", text)
    assert tw and th
    assert (int(tw.group(1)), int(th.group(1))) == (K.TW, K.TH)
    header = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    assert re.search(r"EC_FOCAL_RADIUS_CAP\s*=\s*7\b", header)
    # the stage of the largest launch (radius 7, 8-byte cells, masked, row results) fits well inside 64 KiB
    hr, wide = K.TH + 14, K.TW + 14
    pad = lambda b: (b + 15) // 16 * 16
    assert hr * pad(wide * 8) + hr * pad(wide) + hr * K.TW * 8 + pad(hr * K.TW) <= 40 * 1024


@pytest.mark.parametrize("target", ["test_focal_plan", "test_focal_plan_san"])
def test_the_plan_header_alone_and_under_sanitizers(target):
    """erased-cells_amd/host/test_focal_plan.cpp: the refusals, the tile grid, the staged region and the LDS layout from
    csrc/ec_focal_plan.hpp alone — a stand-alone program, built plainly and with -fsanitize=address,undefined"""
    run_host_program(target)

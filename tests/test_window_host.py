"""ec_window / ec_window_put without a device: the integer resampling rule, the argument checks (all made before any device
work, so they answer the same with no device bound) and the header's citations.  The rule is restated here in exact rational
arithmetic; nothing expected comes from the library."""
import ctypes as C
import os
import re
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (window cells, output cells) along one axis
SMALL = [(w, o) for w in range(1, 41) for o in range(1, 41)]
RATIOS = [(512, 512), (512, 256), (513, 171), (700, 300), (7, 3), (256, 512), (200, 500), (3, 7), (1, 1000), (1000, 1), (999, 1000), (1000, 999)]
# (2 j + 1) * w is an exact multiple of 2 * out for some j: the centre of an output cell falls on a cell boundary of the window
EXACT = [(6, 3), (2, 1), (10, 5), (6, 1), (30, 5), (12, 2), (14, 7), (4, 2), (2 ** 20, 2 ** 19)]
BIG = [(2 ** 31 - 1, 2 ** 31 - 2), (2 ** 31 + 1, 2 ** 30), (2 ** 31 - 1, 2 ** 32 + 3), (2 ** 32 - 1, 2 ** 31 + 5), (2 ** 32 + 1, 2 ** 32 - 1),
       (2 ** 32 + 7, 2 ** 32 + 7), (2 ** 32 + 1, 3), (5, 2 ** 32 + 1), (2 ** 33, 2 ** 31 - 1)]


def rule(j, w, out):
    """floor of the centre of output cell j in window coordinates, (j + 1/2) * w / out, as an exact rational"""
    return (Fraction(2 * j + 1, 2) * Fraction(w, out)).__floor__()


def sample_js(out):
    js = set(range(min(out, 70))) | set(range(max(0, out - 70), out)) | {out // 2, out // 3, (2 * out) // 3}
    for k in range(1, 64):
        js.add((out * k) // 64)
    return sorted(j for j in js if 0 <= j < out)


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def test_index_rule_matches_exact_rational_arithmetic(ec):
    from erased_cells_hip import raster
    for w, out in SMALL + RATIOS + EXACT:
        assert raster.nearest_source_indices(w, out) == [rule(j, w, out) for j in range(out)], (w, out)
    for w, out in BIG:
        for j in sample_js(out):
            assert raster.nearest_source_index(j, w, out) == rule(j, w, out), (w, out, j)
        assert raster.nearest_source_indices(w, out, out - 5, out) == [rule(j, w, out) for j in range(out - 5, out)]


def test_exact_multiples_are_in_the_grid_and_land_on_the_upper_cell():
    """the case a floating-point evaluation may round down: the quotient is an integer and must be taken as it is"""
    from erased_cells_hip import raster
    for w, out in EXACT:
        hits = [j for j in sample_js(out) if ((2 * j + 1) * w) % (2 * out) == 0]
        assert hits, (w, out)
        for j in hits:
            assert raster.nearest_source_index(j, w, out) == ((2 * j + 1) * w) // (2 * out) == rule(j, w, out)
            assert rule(j, w, out) * 2 * out == (2 * j + 1) * w


def test_index_rule_invariants():
    from erased_cells_hip import raster
    for w, out in SMALL + RATIOS + EXACT:
        idx = raster.nearest_source_indices(w, out)
        assert len(idx) == out and idx[0] >= 0 and idx[-1] <= w - 1, (w, out)
        assert all(a <= b for a, b in zip(idx, idx[1:])), (w, out)
        if w == out:
            assert idx == list(range(w))
    for w, out in BIG:
        js = sample_js(out)
        idx = [raster.nearest_source_index(j, w, out) for j in js]
        assert idx[0] >= 0 and idx[-1] <= w - 1 and all(a <= b for a, b in zip(idx, idx[1:])), (w, out)
        if w == out:
            assert idx == js


def _window(L, t=0, src=1, smask=None, cols=0, rows=0, x0=0, y0=0, w=0, h=0, ow=0, oh=0, dst=1, dmask=None):
    return L.ec_window(t, src, smask, cols, rows, x0, y0, w, h, ow, oh, dst, dmask, None)


def _put(L, t=0, tile=1, tmask=None, w=0, h=0, dst=1, dmask=None, cols=0, rows=0, x0=0, y0=0):
    return L.ec_window_put(t, tile, tmask, w, h, dst, dmask, cols, rows, x0, y0, None)


def test_argument_checks_come_before_any_device_work(ec):
    """Every refusal is EC_ERR_ARG with a message — never EC_ERR_NOT_INITIALIZED, never a launch: the pointers are not even valid."""
    import torch
    L, E = ec.lib(), ec._ffi
    ARG = E.EC_ERR_ARG
    big = 2 ** 64 - 1

    def refused(st, *words):
        msg = L.ec_last_error_string().decode()
        assert st == ARG, (st, msg)
        for wd in words:
            assert wd in msg, msg

    # a window that leaves the raster, on every side, including sums that wrap 64 bits
    refused(_window(L, cols=10, rows=10, x0=8, w=3, h=1, ow=3, oh=1), "leaves the raster")
    refused(_window(L, cols=10, rows=10, y0=10, w=1, h=1, ow=1, oh=1), "leaves the raster")
    refused(_window(L, cols=10, rows=10, x0=11, w=0, h=0), "leaves the raster")
    refused(_window(L, cols=10, rows=10, x0=big, w=2, h=1, ow=2, oh=1), "leaves the raster")
    refused(_window(L, cols=10, rows=10, y0=2, w=1, h=big, ow=1, oh=1), "leaves the raster")
    refused(_put(L, cols=10, rows=10, x0=8, w=3, h=1), "leaves the raster")
    refused(_put(L, cols=10, rows=10, y0=big, w=1, h=2), "leaves the raster")
    # exactly one mask
    refused(_window(L, smask=1, cols=4, rows=4, w=2, h=2, ow=2, oh=2), "mask")
    refused(_window(L, dmask=1, cols=4, rows=4, w=2, h=2, ow=2, oh=2), "mask")
    refused(_put(L, tmask=1, cols=4, rows=4, w=2, h=2), "mask")
    refused(_put(L, dmask=1, cols=4, rows=4, w=2, h=2), "mask")
    # a raster whose cell count does not fit 64 bits
    refused(_window(L, cols=2 ** 33, rows=2 ** 33, w=1, h=1, ow=1, oh=1), "overflows")
    refused(_put(L, cols=2 ** 40, rows=2 ** 30, w=1, h=1), "overflows")
    # empty on one side only
    refused(_window(L, cols=4, rows=4, w=2, h=2, ow=0, oh=2), "cannot be read")
    refused(_window(L, cols=4, rows=4, w=2, h=2, ow=2, oh=0), "cannot be read")
    refused(_window(L, cols=4, rows=4, w=0, h=2, ow=2, oh=2), "cannot be read")
    refused(_window(L, cols=4, rows=4, w=2, h=0, ow=1, oh=1), "cannot be read")
    # null buffers of a non-empty call
    refused(_window(L, src=None, cols=4, rows=4, w=2, h=2, ow=2, oh=2), "null")
    refused(_put(L, dst=None, cols=4, rows=4, w=2, h=2), "null")
    # an empty window with an empty output moves nothing and needs nothing — no device either
    assert _window(L, src=None, dst=None, cols=4, rows=4, x0=4, y0=4) == E.EC_OK
    assert _window(L, cols=4, rows=4, x0=1, w=0, h=3, ow=0, oh=7) == E.EC_OK
    assert _window(L, cols=0, rows=0) == E.EC_OK
    assert _put(L, tile=None, dst=None, cols=4, rows=4, x0=2, y0=2) == E.EC_OK
    assert L.ec_window(99, 1, None, 4, 4, 0, 0, 1, 1, 1, 1, 1, None, None) == E.EC_ERR_UNSUPPORTED_TYPE
    if not torch.cuda.is_available():  # a call that passes every check is the first to ask for the device
        assert _window(L, cols=4, rows=4, w=2, h=2, ow=2, oh=2) == E.EC_ERR_NOT_INITIALIZED
        assert _put(L, cols=4, rows=4, w=2, h=2) == E.EC_ERR_NOT_INITIALIZED
        v = C.c_int64(-1)
        assert L.ec_stat_get(b"devices", C.byref(v)) == E.EC_OK and v.value == 0
    assert L.ec_abi_version() == 1


def test_python_mirror_refuses_what_the_reference_cannot_express(ec):
    import numpy as np
    from erased_cells_hip import raster
    band = raster.RasterBand(np.arange(48, dtype=np.uint16).reshape(6, 8), None)
    with pytest.raises(ec.EcError, match="Cubic"):
        band.read_cells((0, 0), (4, 4), (2, 2), "Cubic")
    with pytest.raises(ec.EcError, match="Bilinear"):
        band.read_cells_masked((0, 0), (4, 4), (2, 2), "Bilinear")
    with pytest.raises(ec.EcError, match="negative"):
        band.read_cells((-1, 0), (4, 4), (4, 4), None)
    with pytest.raises(ec.EcError, match="negative"):
        band.read_cells_masked((0, -2), (4, 4), (4, 4), None)
    with pytest.raises(ec.EcError, match="leaves the raster"):
        band.read_cells((5, 0), (4, 4), (4, 4), None)


def test_both_prototypes_cite_the_reference():
    text = open(os.path.join(ROOT, "include", "erased_cells.h")).read()
    for fn in ("ec_window", "ec_window_put"):
        i = text.index("ec_status " + fn + "(")
        comment = text[text.rindex("/*", 0, i):i]
        assert re.search(r"src/gdal/rasterband\.rs:82-125", comment), fn

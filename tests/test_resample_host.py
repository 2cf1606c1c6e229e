"""ec_window_resample without a device: the yardstick itself (tests/resample_ref.py) held to the properties that define the rule, and
the argument checks of the entry point, all of which come before any device work.  Nothing expected comes from the library."""
import ctypes as C
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

import resample_ref as R

# (window cells, output cells) along one axis: whole and fractional factors, up and down, the copy, single cells, the cap
AXES = [(w, o) for w in range(1, 25) for o in range(1, 25)] + [(40, 20), (33, 11), (35, 14), (31, 47), (17, 1), (8, 3), (2, 5), (1, 3),
                                                               (64, 1), (640, 10), (600, 300), (64, 56), (1000, 999), (999, 1000)]
GEOMS = [(40, 8, 20, 4), (33, 7, 11, 7), (35, 7, 14, 3), (31, 5, 47, 8), (17, 3, 1, 1), (8, 8, 8, 3), (2, 2, 5, 5), (1, 1, 3, 2), (64, 2, 1, 2)]


@pytest.fixture(scope="module")
def ec():
    import erased_cells_hip as ec
    return ec


def test_tap_weights_sum_to_the_axis_weight_and_indices_stay_inside_the_window():
    for win, out in AXES:
        for j in range(out):
            av, bl = R.average_taps(j, win, out), R.bilinear_taps(j, win, out)
            assert sum(w for _, w in av) == win // gcd(win, out), (win, out, j)
            assert sum(w for _, w in bl) == 2 * out, (win, out, j)
            for taps in (av, bl):
                assert taps and all(0 <= c <= win - 1 and w > 0 for c, w in taps), (win, out, j, taps)
                assert [c for c, _ in taps] == sorted(c for c, _ in taps)
            assert len(bl) <= 2 and len(av) <= win // out + 2
        # an average covers the window exactly once: per cell, the weights it gets add up to one output cell's worth
        got = {}
        for j in range(out):
            for c, w in R.average_taps(j, win, out):
                got[c] = got.get(c, 0) + w
        assert got == {c: out // gcd(win, out) for c in range(win)}, (win, out)


def test_taps_are_the_overlaps_and_the_centre_weights_in_exact_rationals():
    for win, out in AXES:
        for j in range(out):
            lo, hi = Fraction(j * win, out), Fraction((j + 1) * win, out)  # the output cell in window coordinates
            total = sum(w for _, w in R.average_taps(j, win, out))
            for c, w in R.average_taps(j, win, out):
                assert Fraction(w, total) == (min(hi, c + 1) - max(lo, c)) / (hi - lo), (win, out, j, c)
            centre = Fraction(2 * j + 1, 2) * Fraction(win, out) - Fraction(1, 2)  # in units of cells, measured from the centre of cell 0
            k = centre.__floor__()
            want = {}
            for c, wt in ((k, 1 - (centre - k)), (k + 1, centre - k)):
                if wt:
                    want[min(max(c, 0), win - 1)] = want.get(min(max(c, 0), win - 1), 0) + wt
            got = {}
            for c, w in R.bilinear_taps(j, win, out):
                got[c] = got.get(c, 0) + Fraction(w, 2 * out)
            assert got == want, (win, out, j)


def _cells(dt, cols, rows, seed):
    rng = np.random.default_rng(seed)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=(rows, cols), endpoint=True).astype(dt)


def test_a_whole_factor_is_the_block_mean_and_equal_size_is_the_copy():
    a = _cells(np.uint16, 24, 12, 1)
    for k in (2, 3, 4):
        got, mask = R.resample(R.AVERAGE, a, None, 0, 0, 24, 12, 24 // k, 12 // k)
        for i in range(12 // k):
            for j in range(24 // k):
                block = a[i * k:(i + 1) * k, j * k:(j + 1) * k].astype(object)
                mean = Fraction(int(block.sum()), k * k)
                assert int(got[i, j]) == (mean + Fraction(1, 2)).__floor__(), (k, i, j)
        assert mask.all()
    for alg in (R.BILINEAR, R.AVERAGE):  # cell by cell, not through resample()'s shortcut
        for i in range(5):
            for j in range(7):
                assert R.cell(alg, a, None, 3, 2, 7, 5, 7, 5, i, j) == (a[2 + i, 3 + j], 1)


def _exact(alg, a, x0, y0, w, h, ow, oh, i, j):
    """the same cell in exact rational arithmetic, rounded half away from zero"""
    num, den = 0, 0
    for y, wy in R.taps(alg, i, h, oh):
        for x, wx in R.taps(alg, j, w, ow):
            num += wy * wx * int(a[y0 + y, x0 + x])
            den += wy * wx
    q = Fraction(num, den)
    r = (abs(q) + Fraction(1, 2)).__floor__()
    return r if q >= 0 else -r


def test_the_f64_path_equals_exact_arithmetic_for_small_integer_cells():
    for dt in (np.uint8, np.int16, np.uint16):
        a = _cells(dt, 97, 9, 7)
        for alg in (R.BILINEAR, R.AVERAGE):
            for w, h, ow, oh in GEOMS:
                got, _ = R.resample(alg, a, None, 3, 1, w, h, ow, oh)
                for i in range(oh):
                    for j in range(ow):
                        assert int(got[i, j]) == _exact(alg, a, 3, 1, w, h, ow, oh, i, j), (dt, alg, w, h, ow, oh, i, j)


def test_rounding_and_saturation_of_the_integer_cells():
    f = np.float64
    assert R.to_cell(f(-0.5), np.int8) == -1 and R.to_cell(f(0.5), np.int8) == 1 and R.to_cell(f(0.25), np.int8) == 0
    assert R.to_cell(f(2.0 ** 64), np.uint64) == 2 ** 64 - 1 and R.to_cell(f(-(2.0 ** 63)), np.int64) == -2 ** 63
    assert R.to_cell(f(2.0 ** 63), np.int64) == 2 ** 63 - 1 and R.to_cell(f(300.0), np.uint8) == 255 and R.to_cell(f(-3.0), np.uint8) == 0
    assert R.to_cell(f(0.49999999999999994), np.int8) == 1  # the rule is ONE f64 add: 0.5 - 2^-54 + 0.5 rounds to 1.0
    assert R.to_cell(f(-129.0), np.int8) == -128 and R.to_cell(f(127.5), np.int8) == 127


def test_masked_cells_carry_no_weight():
    a = np.arange(48, dtype=np.float64).reshape(6, 8)
    a[2, 3] = np.nan
    m = np.ones((6, 8), dtype=np.uint8)
    m[2, 3] = 0
    v, ok = R.cell(R.AVERAGE, a, m, 2, 2, 2, 2, 1, 1, 0, 0)  # cells (2..3, 2..3): one invalid NaN among four
    assert ok == 1 and v == np.float64(18 + 26 + 27) / np.float64(3)
    m[:] = 0
    assert R.cell(R.AVERAGE, a, m, 2, 2, 2, 2, 1, 1, 0, 0) == (0.0, 0)
    m[3, 2] = 1
    assert R.cell(R.BILINEAR, a, m, 2, 2, 2, 2, 1, 1, 0, 0) == (a[3, 2], 1)


# ---- the entry point's argument checks, through ctypes, with no device bound
def _rs(L, alg, t=0, src=1, smask=None, cols=0, rows=0, x0=0, y0=0, w=0, h=0, ow=0, oh=0, dst=1, dmask=None):
    return L.ec_window_resample(alg, t, src, smask, cols, rows, x0, y0, w, h, ow, oh, dst, dmask, None)


def _win(L, t=0, src=1, smask=None, cols=0, rows=0, x0=0, y0=0, w=0, h=0, ow=0, oh=0, dst=1, dmask=None):
    return L.ec_window(t, src, smask, cols, rows, x0, y0, w, h, ow, oh, dst, dmask, None)


def test_argument_checks_come_before_any_device_work(ec):
    """Without the feature this test fails at the missing symbol."""
    import torch
    L, E = ec.lib(), ec._ffi
    assert (E.EC_RESAMPLE_NEAREST, E.EC_RESAMPLE_BILINEAR, E.EC_RESAMPLE_AVERAGE, E.EC_WINDOW_MAX_REDUCTION) == (0, 1, 5, 64)
    no_device = not torch.cuda.is_available()
    big = 2 ** 64 - 1

    def refused(st, *words):
        msg = L.ec_last_error_string().decode()
        assert st == E.EC_ERR_ARG, (st, msg)
        for wd in words:
            assert wd in msg, msg

    # an algorithm the library does not have is named: GDAL's Cubic, CubicSpline, Lanczos, Mode, Gauss and a number that is none
    for alg in (2, 3, 4, 6, 7, 99, -1):
        refused(_rs(L, alg, cols=8, rows=8, w=4, h=4, ow=2, oh=2), f"algorithm {alg} ")
        refused(_rs(L, alg, cols=8, rows=8, w=4, h=4, ow=4, oh=4), f"algorithm {alg} ")  # even for the copy
    for alg in (R.BILINEAR, R.AVERAGE):
        # everything ec_window refuses
        refused(_rs(L, alg, cols=10, rows=10, x0=8, w=3, h=1, ow=2, oh=1), "leaves the raster")
        refused(_rs(L, alg, cols=10, rows=10, y0=2, w=1, h=big, ow=1, oh=2), "leaves the raster")
        refused(_rs(L, alg, smask=1, cols=4, rows=4, w=2, h=2, ow=1, oh=1), "one mask without the other")
        refused(_rs(L, alg, dmask=1, cols=4, rows=4, w=2, h=2, ow=1, oh=1), "one mask without the other")
        refused(_rs(L, alg, dmask=1, cols=4, rows=4, w=2, h=2, ow=2, oh=2), "one mask without the other")
        refused(_rs(L, alg, cols=2 ** 33, rows=2 ** 33, w=2, h=2, ow=1, oh=1), "overflows")
        refused(_rs(L, alg, cols=4, rows=4, w=2, h=2, ow=0, oh=2), "cannot be read")
        refused(_rs(L, alg, cols=4, rows=4, w=0, h=2, ow=2, oh=2), "cannot be read")
        refused(_rs(L, alg, src=None, cols=4, rows=4, w=2, h=2, ow=1, oh=1), "null")
        refused(_rs(L, alg, dst=None, cols=4, rows=4, w=2, h=2, ow=3, oh=3), "null")
        assert _rs(L, alg, t=99, cols=4, rows=4, w=2, h=2, ow=1, oh=1) == E.EC_ERR_UNSUPPORTED_TYPE
        # an empty window with an empty output moves nothing and needs nothing
        assert _rs(L, alg, src=None, dst=None, cols=4, rows=4, x0=4, y0=4) == E.EC_OK
        assert _rs(L, alg, cols=4, rows=4, x0=1, w=0, h=3, ow=0, oh=7) == E.EC_OK
        assert _rs(L, alg, cols=0, rows=0) == E.EC_OK
    # the cap of an average: 65 to 1 refused on either axis, 64 to 1 not; bilinear has two taps at any ratio
    refused(_rs(L, R.AVERAGE, cols=65, rows=2, w=65, h=2, ow=1, oh=2), "EC_WINDOW_MAX_REDUCTION", "columns")
    refused(_rs(L, R.AVERAGE, cols=2, rows=130, w=2, h=130, ow=2, oh=2), "EC_WINDOW_MAX_REDUCTION", "rows")
    refused(_rs(L, R.AVERAGE, cols=2 ** 40, rows=1, w=2 ** 40, h=1, ow=3, oh=1), "EC_WINDOW_MAX_REDUCTION")
    # arithmetic that leaves 64 bits: win * out (average), 2 * out * win + out (bilinear), 4 * out_cols * out_rows (bilinear)
    refused(_rs(L, R.AVERAGE, cols=2 ** 33, rows=1, w=2 ** 33, h=1, ow=2 ** 31, oh=1), "win * out", "overflows")
    refused(_rs(L, R.AVERAGE, cols=1, rows=2 ** 32 + 1, w=1, h=2 ** 32 + 1, ow=1, oh=2 ** 32), "win * out", "rows")
    refused(_rs(L, R.BILINEAR, cols=2 ** 32, rows=1, w=2 ** 32, h=1, ow=2 ** 31, oh=1), "2 * out * win + out", "overflows")
    refused(_rs(L, R.BILINEAR, cols=2 ** 31, rows=1, w=2 ** 31, h=1, ow=2 ** 32, oh=1), "2 * out * win + out", "columns")
    refused(_rs(L, R.BILINEAR, cols=2, rows=2, w=2, h=2, ow=2 ** 31, oh=2 ** 31), "total weight", "overflows")
    # more workgroups than a grid holds: one per 1024 slots of 16 bytes, at most 2^31 - 1 of them
    refused(_rs(L, R.BILINEAR, cols=1, rows=1, w=1, h=1, ow=2 ** 40, oh=2 ** 6), "tiles")
    refused(_rs(L, R.AVERAGE, t=9, cols=1, rows=1, w=1, h=1, ow=2 ** 21, oh=2 ** 21), "tiles")
    if no_device:  # a call that passes every check is the first to ask for the device
        assert _rs(L, R.AVERAGE, cols=64, rows=2, w=64, h=2, ow=1, oh=2) == E.EC_ERR_NOT_INITIALIZED
        assert _rs(L, R.AVERAGE, cols=2, rows=128, w=2, h=128, ow=5, oh=2) == E.EC_ERR_NOT_INITIALIZED
        assert _rs(L, R.BILINEAR, cols=650, rows=2, w=650, h=2, ow=1, oh=5) == E.EC_ERR_NOT_INITIALIZED
        assert _rs(L, R.BILINEAR, smask=1, dmask=1, cols=8, rows=8, w=4, h=4, ow=2, oh=2) == E.EC_ERR_NOT_INITIALIZED
        assert _rs(L, R.AVERAGE, cols=8, rows=8, w=4, h=4, ow=4, oh=4) == E.EC_ERR_NOT_INITIALIZED  # the copy
    assert L.ec_abi_version() == 1


def test_nearest_is_refused_and_accepted_exactly_where_ec_window_is(ec):
    import torch
    L = ec.lib()
    big = 2 ** 64 - 1
    calls = [dict(cols=10, rows=10, x0=8, w=3, h=1, ow=3, oh=1), dict(cols=10, rows=10, x0=big, w=2, h=1, ow=2, oh=1),
             dict(smask=1, cols=4, rows=4, w=2, h=2, ow=2, oh=2), dict(dmask=1, cols=4, rows=4, w=2, h=2, ow=1, oh=1),
             dict(cols=2 ** 33, rows=2 ** 33, w=1, h=1, ow=1, oh=1), dict(cols=4, rows=4, w=2, h=2, ow=0, oh=2),
             dict(cols=4, rows=4, w=2, h=0, ow=1, oh=1), dict(src=None, cols=4, rows=4, w=2, h=2, ow=2, oh=2),
             dict(cols=3 * 2 ** 32, rows=1, w=3 * 2 ** 32, h=1, ow=2 ** 33, oh=1),  # beyond the nearest rule's own arithmetic
             dict(t=99, cols=4, rows=4, w=1, h=1, ow=1, oh=1),
             dict(src=None, dst=None, cols=4, rows=4, x0=4, y0=4), dict(cols=0, rows=0), dict(cols=4, rows=4, x0=1, w=0, h=3, ow=0, oh=7)]
    if not torch.cuda.is_available():  # calls that pass every check ask for the device; 650 to 1: nearest neighbour has no cap
        calls += [dict(cols=4, rows=4, w=2, h=2, ow=2, oh=2), dict(cols=8, rows=8, w=4, h=4, ow=2, oh=3), dict(cols=650, rows=2, w=650, h=2, ow=1, oh=1)]
    seen = set()
    for kw in calls:
        a = _win(L, **kw)
        text_a = L.ec_last_error_string().decode() if a else ""
        b = _rs(L, R.NEAREST, **kw)
        text_b = L.ec_last_error_string().decode() if b else ""
        assert (a, text_a) == (b, text_b), kw
        seen.add(a)
    assert {ec._ffi.EC_OK, ec._ffi.EC_ERR_ARG, ec._ffi.EC_ERR_UNSUPPORTED_TYPE} <= seen


def test_python_mirror_names_the_algorithms(ec):
    """resample= is checked by name before any call; RasterBand.read_cells keeps refusing everything but nearest neighbour"""
    buf = ec.CellBuffer(ec.UInt8, 0, None)  # never touched: the name is refused first
    with pytest.raises(ec.EcError, match="Cubic"):
        buf.window(0, (0, 0), (0, 0), (0, 0), resample="Cubic")
    from erased_cells_hip import buffer
    assert buffer.RESAMPLE_ALGS == {"Bilinear": 1, "Average": 5}


def test_the_prototype_cites_the_reference_and_states_the_cap():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "erased_cells.h")).read()
    i = text.index("ec_status ec_window_resample(")
    comment = text[text.rindex("/*", 0, i):i]
    assert re.search(r"src/gdal/rasterband\.rs:82-125", comment)
    assert re.search(r"EC_WINDOW_MAX_REDUCTION\s*=\s*64", text) and "EC_WINDOW_MAX_REDUCTION" in comment
    assert "EC_RESAMPLE_NEAREST = 0, EC_RESAMPLE_BILINEAR = 1, EC_RESAMPLE_AVERAGE = 5" in text

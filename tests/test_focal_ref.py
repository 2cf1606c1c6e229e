"""tests/focal_ref.py, the numpy restatement of the rule of ec_focal / ec_focal_convolve, held to answers that do not come from it: a
scalar loop that transcribes the header's pseudo-code, scipy.ndimage where every order of additions gives the same bits, cells
computed by hand, and a sum whose value depends on the order the rule fixes.  No GPU, nothing from the compiled library (the Landsat
test reads its fixture with the package's pure-Python TIFF reader)."""
import os

import numpy as np
import pytest

import focal_cases as K
import focal_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


def total_order_less(x, y):
    """x before y in the reference's order (src/value.rs:248-265), on scalars, without focal_ref's keys: integers natural; floats by
    sign and magnitude of the bit pattern, which is what total_cmp states"""
    if isinstance(x, (np.floating, float)):
        def parts(v):
            u = int(np.array([v]).view(K.UINT[np.dtype(type(v)).itemsize])[0])
            width = 8 * np.dtype(type(v)).itemsize
            neg, mag = u >> (width - 1), u & ((1 << (width - 1)) - 1)
            return -mag - 1 if neg else mag     # -0.0 -> -1, +0.0 -> 0, more negative the larger the magnitude
        return parts(x) < parts(y)
    return int(x) < int(y)


def scalar_rule(a, mask, rx, ry, op=None, w=None, normalize=False, whole=False):
    """the header's pseudo-code, cell by cell, on numpy float64 SCALARS (each + * / one rounding)"""
    rows, cols = a.shape
    out_dt = np.float64 if (w is not None or op in (R.SUM, R.MEAN)) else a.dtype
    out, valid = np.zeros((rows, cols), dtype=out_dt), np.zeros((rows, cols), dtype=np.uint8)
    with np.errstate(all="ignore"):
        for i in range(rows):
            for j in range(cols):
                acc, wsum, count, best = np.float64(0.0), np.float64(0.0), 0, None
                for y in range(i - ry, i + ry + 1):
                    racc, rw = np.float64(0.0), np.float64(0.0)
                    for x in range(j - rx, j + rx + 1):
                        if not (0 <= y < rows and 0 <= x < cols) or (mask is not None and mask[y, x] == 0):
                            continue
                        c = a[y, x]
                        if w is not None:
                            racc = racc + (np.float64(w[y - i + ry, x - j + rx]) * np.float64(c))
                            rw = rw + np.float64(w[y - i + ry, x - j + rx])
                        elif op in (R.SUM, R.MEAN):
                            racc = racc + np.float64(c)
                        elif best is None or (total_order_less(c, best) if op == R.MIN else total_order_less(best, c)):
                            best = c
                        count += 1
                    acc = acc + racc
                    wsum = wsum + rw
                ok = count == (2 * rx + 1) * (2 * ry + 1) if whole else count > 0
                if w is not None:
                    r = acc / wsum if normalize else acc
                    ok = ok and not (normalize and wsum == 0.0)
                elif op == R.SUM:
                    r = acc
                elif op == R.MEAN:
                    r = acc / np.float64(count)
                else:
                    r = best
                if ok:
                    out[i, j], valid[i, j] = r, 1
    return out, valid


SMALL = [(9, 7), (1, 1), (4, 1), (1, 5), (3, 3)]
SMALL_RADII = [(0, 0), (1, 1), (2, 1), (1, 3), (7, 7)]


@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
@pytest.mark.parametrize("ct", range(10))
def test_against_the_scalar_transcription(ct, masked):
    for k, (cols, rows) in enumerate(SMALL):
        a = K.raster_cells(ct, cols, rows, 0x5CA1 + ct + k)
        m = K.mask_bytes("hashed", cols, rows, 0x77 + k) if masked else None
        for rx, ry in SMALL_RADII[:3] if k else SMALL_RADII:
            for whole in (False, True):
                for op in (R.SUM, R.MEAN, R.MIN, R.MAX):
                    got, gv = R.focal(op, a, m, rx, ry, whole)
                    exp, ev = scalar_rule(a, m, rx, ry, op=op, whole=whole)
                    assert same(got, exp) and np.array_equal(gv, ev), (ct, cols, rows, rx, ry, op, whole)
                for normalize in (False, True):
                    w = K.weights(rx, ry)
                    got, gv = R.convolve(a, m, w, normalize, whole)
                    exp, ev = scalar_rule(a, m, rx, ry, w=w, normalize=normalize, whole=whole)
                    assert same(got, exp) and np.array_equal(gv, ev), (ct, cols, rows, rx, ry, normalize, whole)


def test_total_order_of_floats_in_the_transcription_and_the_keys():
    for dt in (np.float32, np.float64):
        v = np.array([-np.nan, -np.inf, -1.5, -0.0, 0.0, 1.5, np.inf, np.nan], dtype=dt)
        assert np.signbit(v[0]) and not np.signbit(v[-1])
        k = R.order_keys(v)
        assert (k[1:] > k[:-1]).all()
        assert same(R.cells_of_keys(k, dt), v)
        for i in range(len(v) - 1):
            assert total_order_less(v[i], v[i + 1]) and not total_order_less(v[i + 1], v[i])
    for dt in (np.uint64, np.int64, np.int8, np.uint8):
        info = np.iinfo(dt)
        v = np.array([info.min, info.min + 1, info.max - 1, info.max], dtype=dt)
        k = R.order_keys(v)
        assert (k[1:] > k[:-1]).all() and same(R.cells_of_keys(R.order_keys(v), dt), v)


@pytest.mark.parametrize("ct", (0, 1, 2, 4, 5, 6))
def test_against_scipy_ndimage_where_sums_are_exact(ct):
    """integer cells of at most 32 bits: every partial sum is an integer below 2^53, so any order of additions gives the same bits"""
    ndi = pytest.importorskip("scipy.ndimage")
    cols, rows = 23, 17
    a = K.raster_cells(ct, cols, rows, 0x5C1 + ct)
    af = a.astype(np.float64)
    for rx, ry in ((1, 1), (2, 1), (1, 3), (7, 7), (0, 2)):
        ones = np.ones((2 * ry + 1, 2 * rx + 1))
        got, gv = R.focal(R.SUM, a, None, rx, ry)
        assert same(got, ndi.correlate(af, ones, mode="constant", cval=0.0)) and gv.all()
        count = ndi.correlate(np.ones((rows, cols)), ones, mode="constant", cval=0.0)
        got, _ = R.focal(R.MEAN, a, None, rx, ry)
        assert same(got, ndi.correlate(af, ones, mode="constant", cval=0.0) / count)
        _, whole = R.focal(R.SUM, a, None, rx, ry, whole=True)
        assert np.array_equal(whole, (count == ones.size).astype(np.uint8))
        w = np.round(K.weights(rx, ry) * 3.0)   # small integers: products and sums stay exact
        got, _ = R.convolve(a, None, w)
        assert same(got, ndi.correlate(af, w, mode="constant", cval=0.0) + 0.0)
        # a replicated edge cell is always inside the clipped footprint, so "nearest" gives the clipped extremes
        got, _ = R.focal(R.MIN, a, None, rx, ry)
        assert same(got, ndi.minimum_filter(a, size=(2 * ry + 1, 2 * rx + 1), mode="nearest"))
        got, _ = R.focal(R.MAX, a, None, rx, ry)
        assert same(got, ndi.maximum_filter(a, size=(2 * ry + 1, 2 * rx + 1), mode="nearest"))
        # masked sums: the masked-out cells as zeros, the count from the mask itself
        m = K.mask_bytes("hashed", cols, rows, 0x99 + rx)
        got, gv = R.focal(R.SUM, a, m, rx, ry)
        cnt = ndi.correlate(m.astype(np.float64), ones, mode="constant", cval=0.0)
        exp = np.where(cnt > 0, ndi.correlate(af * m, ones, mode="constant", cval=0.0), 0.0)
        assert same(got, exp) and np.array_equal(gv, (cnt > 0).astype(np.uint8))


def test_a_single_one_gives_the_footprint_clipped_at_edges_and_corners():
    cols, rows, rx, ry = 9, 7, 2, 1
    for y, x in ((3, 4), (0, 0), (0, 8), (6, 0), (6, 8), (0, 4), (3, 0), (6, 7), (1, 1)):
        a = np.zeros((rows, cols), dtype=np.uint8)
        a[y, x] = 1
        foot = np.zeros((rows, cols))
        foot[max(0, y - ry):y + ry + 1, max(0, x - rx):x + rx + 1] = 1.0
        got, gv = R.focal(R.SUM, a, None, rx, ry)
        assert np.array_equal(got, foot) and gv.all(), (y, x)
        got, _ = R.focal(R.MAX, a, None, rx, ry)
        assert np.array_equal(got, foot.astype(np.uint8)), (y, x)
        # the weight that meets the one on its way through the footprint: a correlation shows the weights flipped
        w = np.arange(15, dtype=np.float64).reshape(3, 5) + 1.0
        got, _ = R.convolve(a, None, w)
        for i in range(rows):
            for j in range(cols):
                dy, dx = y - i + ry, x - j + rx
                assert got[i, j] == (w[dy, dx] if 0 <= dy < 3 and 0 <= dx < 5 else 0.0), (y, x, i, j)


def test_three_by_three_mean_of_the_landsat_band_by_hand():
    """L8-Elkton-VA-B4.tiff, 186 x 169 UInt16 cells: the top-left corner (4 taps), an interior cell (9) and the bottom-right corner (4),
    their neighbours written out and added by hand"""
    from erased_cells_hip import raster   # the package's TIFF reader: plain Python, neither the compiled library nor a device
    a = raster.RasterBand.open(os.path.join(GOLDEN, "L8-Elkton-VA-B4.tiff")).cells
    assert a.shape == (169, 186) and a.dtype == np.uint16
    assert a[0:2, 0:2].tolist() == [[6697, 6898], [6772, 6715]]
    assert a[99:102, 56:59].tolist() == [[6599, 6586, 6573], [6632, 6621, 6616], [6620, 6640, 6656]]
    assert a[167:169, 184:186].tolist() == [[6495, 6534], [6494, 6530]]
    got, gv = R.focal(R.MEAN, a, None, 1, 1)
    assert gv.all()
    assert got[0, 0] == 27082 / 4 == 6770.5                 # 6697 + 6898 + 6772 + 6715
    assert got[100, 57] == 59543 / 9                        # 19758 + 19869 + 19916
    assert got[168, 185] == 26053 / 4 == 6513.25            # 6495 + 6534 + 6494 + 6530
    sums, _ = R.focal(R.SUM, a, None, 1, 1)
    assert (sums[0, 0], sums[100, 57], sums[168, 185]) == (27082.0, 59543.0, 26053.0)


def test_the_sum_is_taken_row_by_row_then_down_the_rows():
    """[1e16, 1, -1e16, 1]-style rows: each row sums to 1.0 on its own (1e16 + 1 = 1e16, - 1e16 = 0, + 1 = 1), so rows-then-columns
    gives 3.0 for three of them; column by column the ones are absorbed: (3e16) + (3.0) + (-3e16) + 3.0 = 3.0 ... but transposed
    operands give another value, and a flat loop without racc gives 1.0"""
    row = np.array([1e16, 1.0, -1e16, 1.0])
    a = np.tile(row, (3, 1))
    got, _ = R.focal(R.SUM, a, None, 3, 1)
    centre = got[1, 1]   # columns 0 .. 3 (clipped on the left), rows 0 .. 2
    assert centre == 3.0
    flat = np.float64(0.0)
    for y in range(3):
        for x in range(4):
            flat = flat + a[y, x]
    assert flat == 1.0 and flat != centre
    column_major = np.float64(0.0)
    for x in range(4):
        cacc = np.float64(0.0)
        for y in range(3):
            cacc = cacc + a[y, x]
        column_major = column_major + cacc
    assert column_major != centre
    b = np.array([[1e16, 1.0], [-1e16, 1.0]])
    rows_first, _ = R.focal(R.SUM, b, None, 1, 1)
    assert rows_first[0, 0] == (1e16 + 1.0) + (-1e16 + 1.0) == 0.0
    assert (1e16 + -1e16) + (1.0 + 1.0) == 2.0   # what columns-then-rows would give

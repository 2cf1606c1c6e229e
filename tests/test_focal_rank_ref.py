"""tests/focal_rank_ref.py, the numpy statement of ec_focal_rank / ec_focal_majority, held to: a scalar transcription of the header's
rule (Python's `sorted` on the keys of the taps, one cell at a time), composite_rank_ref over the stack of the footprint's shifted
copies with off-raster cells as cleared mask bytes, focal_ref's MIN and MAX at num = 0 and num = den, scipy.ndimage's median and rank
filters on interior cells, collections.Counter for the majority, and cells worked out by hand.  No GPU."""
from collections import Counter

import numpy as np
import pytest

import composite_rank_ref as CRR
import focal_cases as FC
import focal_rank_cases as K
import focal_rank_ref as R
import focal_ref as FR

NAMES = CRR.NAMES
SMALL = [(1, 1), (2, 5), (9, 4), (23, 11)]
SMALL_RADII = [(0, 0), (1, 0), (1, 1), (2, 1), (0, 2), (3, 4), (7, 1)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(K.UINT[a.dtype.itemsize])


def same(got, exp):
    return got[0].dtype == exp[0].dtype and np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(got[1], exp[1])


def scalar_taps(a, mask, rx, ry, i, j):
    """the header: the taps of output cell (i, j) as (key, bits), rows ascending, columns ascending within a row"""
    rows, cols = a.shape
    key, word = R.order_key(a), R.words(a)
    out = []
    for y in range(i - ry, i + ry + 1):
        for x in range(j - rx, j + rx + 1):
            if 0 <= y < rows and 0 <= x < cols and (mask is None or mask[y, x] != 0):
                out.append((int(key[y, x]), int(word[y, x])))
    return out


def scalar(a, mask, rx, ry, whole, keep):
    """`keep(sorted taps) -> bits` for every valid cell"""
    out, valid = np.zeros(a.shape, np.uint64), np.zeros(a.shape, np.uint8)
    for i in range(a.shape[0]):
        for j in range(a.shape[1]):
            t = sorted(scalar_taps(a, mask, rx, ry, i, j))
            if (len(t) == (2 * rx + 1) * (2 * ry + 1)) if whole else (len(t) > 0):
                out[i, j], valid[i, j] = keep(t), 1
    return out.astype(K.UINT[a.dtype.itemsize]).view(a.dtype), valid


def scalar_rank(a, mask, rx, ry, num, den, method, whole):
    def keep(t):
        c = len(t)
        r = (num * (c - 1)) // den if method == R.LOWER else (num * (c - 1) + den - 1) // den
        return t[r][1]
    return scalar(a, mask, rx, ry, whole, keep)


def scalar_majority(a, mask, rx, ry, whole):
    def keep(t):
        counts = Counter(k for k, _ in t)
        most = max(counts.values())
        least = min(k for k, c in counts.items() if c == most)
        return dict(t)[least]
    return scalar(a, mask, rx, ry, whole, keep)


def inputs(ct, cols, rows, seed):
    yield K.rank_raster(ct, cols, rows, seed), None
    yield K.rank_raster(ct, cols, rows, seed + 1), K.mask_bytes("hashed", cols, rows, seed)
    yield K.class_raster(ct, cols, rows, seed + 2), K.mask_bytes("single-zero", cols, rows, seed)


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_against_the_scalar_transcription(ct):
    for cols, rows in SMALL:
        for rx, ry in SMALL_RADII:
            for a, m in inputs(ct, cols, rows, 0x51 + ct):
                od = R.ordered(a, m, rx, ry)
                for whole in (False, True):
                    for num, den, method in K.QS + [(1, 3, R.UPPER), (65534, 65535, R.LOWER)]:
                        assert same(R.pick(od, num, den, method, whole, a.dtype), scalar_rank(a, m, rx, ry, num, den, method, whole)), (cols, rows, rx, ry, num, den, method, whole)
                    assert same(R.majority_pick(od, whole, a.dtype), scalar_majority(a, m, rx, ry, whole)), (cols, rows, rx, ry, whole)


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_against_composite_rank_over_the_shifted_copies(ct):
    """the footprint as a stack: layer k is the raster shifted by tap k, its mask cleared where the shifted cell lies off the raster or
    is masked out.  Bit for bit at every cell, edges included."""
    for cols, rows in [(23, 11), (K.TW + 1, 3)]:
        for rx, ry in [(1, 1), (2, 1), (0, 3), (3, 4)]:
            for a, m in inputs(ct, cols, rows, 0x61 + ct):
                layer_bits, _, tap = R.gather(a, m, rx, ry)
                layers = [lb.ravel().astype(K.UINT[a.dtype.itemsize]).view(a.dtype) for lb in layer_bits]
                masks = [t.ravel().astype(np.uint8) for t in tap]
                full = len(layers)
                for whole in (False, True):
                    for num, den, method in K.QS:
                        cells, mask, _ = CRR.composite_rank(ct, layers, masks, num, den, method, full if whole else 1)
                        got = R.focal_rank(a, m, rx, ry, num, den, method, whole)
                        assert same((got[0].ravel(), got[1].ravel()), (cells, mask)), (cols, rows, rx, ry, num, den, method, whole)


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_the_ends_are_focal_min_and_max(ct):
    for cols, rows in [(23, 11), (K.TW + 1, K.TH + 1)]:
        for rx, ry in [(0, 0), (1, 1), (2, 1), (7, 1), (3, 4)]:
            for a, m in inputs(ct, cols, rows, 0x71 + ct):
                for whole in (False, True):
                    for method in (R.LOWER, R.UPPER):
                        assert same(R.focal_rank(a, m, rx, ry, 0, 5, method, whole), FR.focal(FR.MIN, a, m, rx, ry, whole))
                        assert same(R.focal_rank(a, m, rx, ry, 5, 5, method, whole), FR.focal(FR.MAX, a, m, rx, ry, whole))


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_against_scipy_on_interior_cells(ct):
    ndimage = pytest.importorskip("scipy.ndimage")
    cols, rows = 41, 29
    a = FC.raster_cells(ct, cols, rows, 0x81 + ct)
    if a.dtype.kind in "iu" and a.dtype.itemsize == 8:
        a = a >> a.dtype.type(11)   # scipy's filters take 64-bit integers through doubles: values of at most 53 bits come through exactly
    for rx, ry in [(1, 1), (2, 1), (1, 3), (3, 3)]:
        size, n = (2 * ry + 1, 2 * rx + 1), (2 * rx + 1) * (2 * ry + 1)
        inner = (slice(ry, rows - ry), slice(rx, cols - rx))
        med = ndimage.median_filter(a, size=size, mode="constant")
        for method in (R.LOWER, R.UPPER):     # n is odd: both medians are the middle one
            got = R.focal_rank(a, None, rx, ry, 1, 2, method)[0]
            assert np.array_equal(got[inner], med[inner]), (rx, ry)
        for r in (0, 1, n // 3, n - 2, n - 1):
            got = R.focal_rank(a, None, rx, ry, r, n - 1, R.LOWER)[0]   # r / (n - 1) is exact: position r
            assert np.array_equal(got[inner], ndimage.rank_filter(a, r, size=size, mode="constant")[inner]), (rx, ry, r)


@pytest.mark.parametrize("ct", range(10), ids=NAMES)
def test_the_majority_against_counter(ct):
    """every cell's footprint counted with collections.Counter over (key, bits) taken straight from the raster"""
    for cols, rows in [(23, 11), (7, 3)]:
        a = K.class_raster(ct, cols, rows, 0x91 + ct)
        m = K.mask_bytes("hashed", cols, rows, 0x92)
        key, word = R.order_key(a), bits(a)
        for mask in (None, m):
            for rx, ry in [(1, 1), (2, 2), (3, 4), (0, 7)]:
                got, gv = R.focal_majority(a, mask, rx, ry)
                for i in range(rows):
                    for j in range(cols):
                        ys, xs = slice(max(0, i - ry), i + ry + 1), slice(max(0, j - rx), j + rx + 1)
                        on = np.ones(key[ys, xs].shape, bool) if mask is None else mask[ys, xs] != 0
                        c = Counter(zip(key[ys, xs][on].tolist(), word[ys, xs][on].tolist()))
                        assert gv[i, j] == (1 if c else 0)
                        if c:
                            most = max(c.values())
                            assert int(bits(got)[i, j]) == min(kw for kw, n in c.items() if n == most)[1], (i, j, rx, ry)
                        else:
                            assert int(bits(got)[i, j]) == 0


def test_cells_worked_out_by_hand():
    a = np.array([[5, 1, 9, 3],
                  [7, 2, 8, 4],
                  [6, 0, 200, 3]], np.uint8)
    # (1, 1), radius (1, 1): all nine of 5 1 9 7 2 8 6 0 200 -> sorted 0 1 2 5 6 7 8 9 200: the median is 6, the outlier 200 is gone
    assert R.focal_rank(a, None, 1, 1, 1, 2, R.LOWER)[0][1, 1] == 6 == R.focal_rank(a, None, 1, 1, 1, 2, R.UPPER)[0][1, 1]
    # the corner (0, 0): the clipped footprint 5 1 7 2 -> sorted 1 2 5 7, c = 4: lower median r = 3 // 2 = 1 -> 2, upper r = 2 -> 5
    assert R.focal_rank(a, None, 1, 1, 1, 2, R.LOWER)[0][0, 0] == 2 and R.focal_rank(a, None, 1, 1, 1, 2, R.UPPER)[0][0, 0] == 5
    # 9/10 of c - 1 = 3 is 2.7: lower 2 -> 5, upper 3 -> 7; under WHOLE the corner is invalid
    assert R.focal_rank(a, None, 1, 1, 9, 10, R.LOWER)[0][0, 0] == 5 and R.focal_rank(a, None, 1, 1, 9, 10, R.UPPER)[0][0, 0] == 7
    out, valid = R.focal_rank(a, None, 1, 1, 1, 2, R.LOWER, whole=True)
    assert valid.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0]] and out[0, 0] == 0 and out[1, 2] == 3
    # with (0, 0) and (1, 1) masked out the corner's taps are 1 7 -> lower 1, upper 7: r follows the clipped count, 2
    m = np.ones(a.shape, np.uint8)
    m[0, 0] = m[1, 1] = 0
    assert R.focal_rank(a, m, 1, 1, 1, 2, R.LOWER)[0][0, 0] == 1 and R.focal_rank(a, m, 1, 1, 1, 2, R.UPPER)[0][0, 0] == 7
    # the footprint never wraps: radius (1, 0) at (1, 0) sees 7 2, not the 3 that ends the row above
    assert R.focal_rank(a, None, 1, 0, 0, 1, R.LOWER)[0][1, 0] == 2

    c = np.array([[1, 1, 2, 2],
                  [3, 1, 2, 3],
                  [3, 3, 2, 2]], np.uint8)
    got, valid = R.focal_majority(c, None, 1, 1)
    # (1, 1): 1 1 2 3 1 2 3 3 2 -> three each of 1, 2 and 3: the least, 1.  (1, 2): 1 2 2 1 2 3 3 2 2 -> five 2s, a strict majority
    assert got[1, 1] == 1 and got[1, 2] == 2 and valid.all()
    # (0, 0): 1 1 3 1 -> 1.   (2, 0): 3 1 3 3 -> 3.   (0, 3): 2 2 2 3 -> 2
    assert got[0, 0] == 1 and got[2, 0] == 3 and got[0, 3] == 2
    f = np.array([[0.0, -0.0, -0.0, np.nan, 1.0]], np.float32)
    got, _ = R.focal_majority(f, None, 2, 0)
    # (0, 2) sees all five: -0.0 twice, every other key once — -0.0 and 0.0 are different keys
    assert bits(got)[0, 2] == 0x80000000
    # (0, 0) sees 0.0 -0.0 -0.0 -> -0.0;  (0, 4) sees -0.0 nan 1.0, one each -> the least key, -0.0
    assert bits(got)[0, 0] == 0x80000000 and bits(got)[0, 4] == 0x80000000
    # (0, 3), radius (1, 0): -0.0 nan 1.0 one each -> -0.0; without the -0.0 (masked out) nan and 1.0 tie: 1.0 < +NaN in the total order
    assert bits(R.focal_majority(f, np.array([[1, 1, 0, 1, 1]], np.uint8), 1, 0)[0])[0, 3] == 0x3F800000

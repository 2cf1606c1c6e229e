"""The rule of ec_focal / ec_focal_convolve (include/erased_cells.h) restated in numpy, for the tests to compare the kernels with.

Shifted views of the raster padded by the radius: tap (dy, dx) of every output cell at once.  Taps are taken in the rule's order —
rows ascending, columns ascending within a row, one partial sum `racc` per footprint row — and a cell that is no tap (outside the
raster, or masked out) never enters an addition: `np.where` keeps the sum as it was, whatever the cell holds.  Every step is one
numpy operation on float64 arrays, so each is individually rounded (numpy does not fuse a multiply into an add).

Imports nothing from the library.  tests/test_focal_ref.py holds this file to independent answers.
"""
import numpy as np

SUM, MEAN, MIN, MAX = range(4)
OPS = {"sum": SUM, "mean": MEAN, "min": MIN, "max": MAX}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
SINT = {4: np.int32, 8: np.int64}


def result_dtype(op, dtype):
    return np.dtype(np.float64) if op in (SUM, MEAN) else np.dtype(dtype)


def order_keys(a):
    """int64 keys whose natural order is the reference's total order of the cells (src/value.rs:248-265): integers natural,
    floats by total_cmp (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN)"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        b = a.view(SINT[a.dtype.itemsize]).astype(np.int64)
        width = 8 * a.dtype.itemsize
        flip = np.int64((1 << (width - 1)) - 1)
        return np.where(b < 0, b ^ flip, b)
    if a.dtype == np.uint64:
        return (a ^ np.uint64(1 << 63)).view(np.int64)
    return a.astype(np.int64)


def cells_of_keys(k, dtype):
    """the inverse of order_keys: the cells, bit for bit"""
    dtype = np.dtype(dtype)
    k = np.asarray(k, dtype=np.int64)
    if dtype.kind == "f":
        flip = np.int64((1 << (8 * dtype.itemsize - 1)) - 1)
        b = np.where(k < 0, k ^ flip, k)
        return b.astype(SINT[dtype.itemsize]).view(dtype)
    if dtype == np.uint64:
        return k.view(np.uint64) ^ np.uint64(1 << 63)
    return k.astype(dtype)


def _padded(a, mask, rx, ry):
    """(cells, is-a-tap) of the raster with a border of ry rows and rx columns that hold no tap"""
    rows, cols = a.shape
    p = np.zeros((rows + 2 * ry, cols + 2 * rx), dtype=a.dtype)
    t = np.zeros(p.shape, dtype=bool)
    p[ry:ry + rows, rx:rx + cols] = a
    t[ry:ry + rows, rx:rx + cols] = True if mask is None else (np.asarray(mask).reshape(rows, cols) != 0)
    return p, t


def _finish(r, count, full, whole, out_dtype, extra_valid=None):
    valid = (count == full) if whole else (count > 0)
    if extra_valid is not None:
        valid = valid & extra_valid
    out = np.zeros(r.shape, dtype=out_dtype)   # an invalid cell: all-zero bits
    out[valid] = r[valid]
    return out, valid.astype(np.uint8)


def focal(op, a, mask, rx, ry, whole=False):
    """-> (rows x cols cells of result_dtype(op, a.dtype), rows x cols mask bytes)"""
    a = np.asarray(a)
    rows, cols = a.shape
    p, t = _padded(a, mask, rx, ry)
    count = np.zeros((rows, cols), dtype=np.int64)
    full = (2 * rx + 1) * (2 * ry + 1)
    if op in (SUM, MEAN):
        acc = np.zeros((rows, cols), dtype=np.float64)
        with np.errstate(all="ignore"):
            for dy in range(2 * ry + 1):
                racc = np.zeros((rows, cols), dtype=np.float64)
                for dx in range(2 * rx + 1):
                    tap = t[dy:dy + rows, dx:dx + cols]
                    racc = np.where(tap, racc + p[dy:dy + rows, dx:dx + cols].astype(np.float64), racc)
                    count += tap
                acc = acc + racc
            r = acc / count.astype(np.float64) if op == MEAN else acc
        return _finish(r, count, full, whole, np.float64)
    assert op in (MIN, MAX), op
    keys = order_keys(p)
    if op == MIN:
        keys = ~keys
    best = np.full((rows, cols), np.iinfo(np.int64).min, dtype=np.int64)
    for dy in range(2 * ry + 1):
        for dx in range(2 * rx + 1):
            tap = t[dy:dy + rows, dx:dx + cols]
            k = keys[dy:dy + rows, dx:dx + cols]
            best = np.where(tap & (k > best), k, best)
            count += tap
    r = cells_of_keys(~best if op == MIN else best, a.dtype)
    return _finish(r, count, full, whole, a.dtype)


def convolve(a, mask, weights, normalize=False, whole=False):
    """weights: (2 ry + 1) x (2 rx + 1); weight [dy][dx] meets cell (i - ry + dy, j - rx + dx) -> (f64 cells, mask bytes)"""
    a = np.asarray(a)
    w = np.asarray(weights, dtype=np.float64)
    assert w.ndim == 2 and w.shape[0] % 2 == 1 and w.shape[1] % 2 == 1, w.shape
    ry, rx = w.shape[0] // 2, w.shape[1] // 2
    rows, cols = a.shape
    p, t = _padded(a, mask, rx, ry)
    count = np.zeros((rows, cols), dtype=np.int64)
    acc = np.zeros((rows, cols), dtype=np.float64)
    wsum = np.zeros((rows, cols), dtype=np.float64)
    with np.errstate(all="ignore"):
        for dy in range(2 * ry + 1):
            racc = np.zeros((rows, cols), dtype=np.float64)
            rw = np.zeros((rows, cols), dtype=np.float64)
            for dx in range(2 * rx + 1):
                tap = t[dy:dy + rows, dx:dx + cols]
                term = w[dy, dx] * p[dy:dy + rows, dx:dx + cols].astype(np.float64)
                racc = np.where(tap, racc + term, racc)
                rw = np.where(tap, rw + w[dy, dx], rw)
                count += tap
            acc = acc + racc
            wsum = wsum + rw
        r = acc / wsum if normalize else acc
    return _finish(r, count, w.size, whole, np.float64, (wsum != 0.0) if normalize else None)

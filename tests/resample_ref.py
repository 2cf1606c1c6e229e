"""The rule of ec_window_resample (include/erased_cells.h) in Python integers and np.float64 scalars: the yardstick of
test_resample_host.py and test_gpu_resample.py.  It shares no code with the library.  Every +, * and / on values is one np.float64
operation (IEEE, individually rounded: numpy scalars never fuse), weights and their sums are Python integers."""
from math import gcd

import numpy as np

NEAREST, BILINEAR, AVERAGE = 0, 1, 5  # GDAL's GRIORA_* numbers
MAX_REDUCTION = 64


def average_taps(j, win, out):
    g = gcd(win, out)
    win, out = win // g, out // g
    lo, hi = j * win, (j + 1) * win
    return [(c, min((c + 1) * out, hi) - max(c * out, lo)) for c in range(lo // out, (hi - 1) // out + 1)]


def bilinear_taps(j, win, out):
    t = (2 * j + 1) * win + out
    k, f = divmod(t, 2 * out)
    taps = [(k - 1, 2 * out - f), (k, f)]
    return [(min(max(c, 0), win - 1), w) for c, w in taps if w != 0]


def taps(alg, j, win, out):
    return average_taps(j, win, out) if alg == AVERAGE else bilinear_taps(j, win, out)


def _int_limits(dt):
    info = np.iinfo(dt)
    return int(info.min), int(info.max)


def to_cell(r, dt):
    """r (np.float64) as a cell of dtype dt"""
    dt = np.dtype(dt)
    if dt == np.float64:
        return np.float64(r)
    if dt == np.float32:
        with np.errstate(all="ignore"):
            return np.float32(r)
    with np.errstate(all="ignore"):
        v = np.trunc(r + np.copysign(np.float64(0.5), r))
    lo, hi = _int_limits(dt)
    if np.isnan(v):
        return dt.type(0)
    if v >= np.float64(hi):  # the 64-bit limits compare in f64, where they are 2^63 and 2^64
        return dt.type(hi)
    if v <= np.float64(lo):
        return dt.type(lo)
    return dt.type(int(v))


def cell(alg, a, m, x0, y0, w, h, ow, oh, i, j):
    """(value, valid) of output cell (row i, column j) of the window (x0, y0) + w x h of the 2-D array a, delivered as ow x oh; m: None
    or the 2-D mask of a"""
    acc, wsum = np.float64(0.0), 0
    with np.errstate(all="ignore"):
        for y, wy in taps(alg, i, h, oh):
            racc, rw = np.float64(0.0), 0
            for x, wx in taps(alg, j, w, ow):
                if m is None or m[y0 + y, x0 + x] != 0:
                    racc = racc + np.float64(wx) * np.float64(a[y0 + y, x0 + x])
                    rw += wx
            acc = acc + np.float64(wy) * racc
            wsum += wy * rw
        if wsum == 0:
            return a.dtype.type(0), 0
        return to_cell(acc / np.float64(wsum), a.dtype), 1


def resample(alg, a, m, x0, y0, w, h, ow, oh):
    """(values oh x ow, mask oh x ow of uint8) — every cell by the loop above; for the small shapes of the tests"""
    out, om = np.zeros((oh, ow), dtype=a.dtype), np.zeros((oh, ow), dtype=np.uint8)
    if (w, h) == (ow, oh):
        out[...] = a[y0:y0 + h, x0:x0 + w]
        om[...] = 1 if m is None else m[y0:y0 + h, x0:x0 + w]
        return out, om
    for i in range(oh):
        for j in range(ow):
            out[i, j], om[i, j] = cell(alg, a, m, x0, y0, w, h, ow, oh, i, j)
    return out, om
